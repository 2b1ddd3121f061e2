"""Rate of the list-output decode (decode_scl_llr_list_dev) beside the decode it extends -> profiles/list/rates.json.

Device-resident, synthetic workload (Eb/N0 2 dB). Shapes: the headline N = 2048, K = 1024, CRC 16, L = 32; N = 1024, K = 512, CRC 8
at L = 8 and at L = 2; each at B = 8 192 and 65 536. Three variants, alternated inside one process:
  list        decode_scl_llr_list_dev with all five outputs;
  mode1       decode_scl_llr_dev under polar_set_mode(1), batch kernel (lat_max_b = -1): the same arithmetic, the fair parent;
  auto        decode_scl_llr_dev under automatic mode (the exp-domain kernels from lists of 3 on).
One warm-up round, `--rounds` timed rounds of `--calls` back-to-back calls between HIP events; median [min - max] in M codewords / s.
Per shape also, at B = 8 192 and two Eb/N0 points, through list_find_dev: list_miss = the sent word is in no row of the list (the
genie-CRC bound of that list size), bler = the row decode_scl_llr returns is not the sent word.
Each shape runs in a child process of its own under a time limit; a failed child ends the run.

    python tools/list_rates.py [--out profiles/list/rates.json] [--rounds 3] [--calls 2]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "headline_l32": dict(n=11, K=1024, crc=16, L=32, limit=300),
    "n1024_l8": dict(n=10, K=512, crc=8, L=8, limit=180),
    "n1024_l2": dict(n=10, K=512, crc=8, L=2, limit=180),
}
BATCHES = (8192, 65536)
EBNO_POINTS = (1.0, 2.0)
VARIANTS = ("list", "mode1", "auto")


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": xs}


def one(name, rounds, calls):
    import ctypes as C
    import torch
    import polar_amd
    c = CONFIGS[name]
    n, K, crc, L = c["n"], c["K"], c["crc"], c["L"]
    N = 1 << n
    torch.cuda.set_device(0)
    C.CDLL(None).srand(C.c_uint(1))
    g = polar_amd.PolarCode(n, K, 0.32, crc)
    Bmax = max(BATCHES)
    llr = torch.empty((Bmax, N), dtype=torch.float64, device="cuda")
    info = torch.empty((Bmax, K), dtype=torch.uint8, device="cuda")
    cand = torch.zeros((Bmax, L, K), dtype=torch.uint8, device="cuda")
    pm = torch.zeros((Bmax, L), dtype=torch.float64, device="cuda")
    ok = torch.zeros((Bmax, L), dtype=torch.uint8, device="cuda")
    na = torch.zeros(Bmax, dtype=torch.int32, device="cuda")
    win = torch.zeros(Bmax, dtype=torch.int32, device="cuda")
    out = torch.zeros((Bmax, K), dtype=torch.uint8, device="cuda")
    dpm = torch.zeros(Bmax, dtype=torch.float64, device="cuda")
    rank = torch.zeros(Bmax, dtype=torch.int32, device="cuda")
    g.debug_set("lat_max_b", -1)

    def call(v, B):
        if v == "list":
            g.decode_scl_llr_list_dev(llr.data_ptr(), "f64", B, L, cand.data_ptr(), pm.data_ptr(), ok.data_ptr(), na.data_ptr(), win.data_ptr())
        else:
            g.decode_scl_llr_dev(llr.data_ptr(), B, L, out.data_ptr(), dpm.data_ptr())

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {"config": {k: c[k] for k in ("n", "K", "crc", "L")}, "extra_output_bytes_per_codeword": L * K + 9 * L + 8, "rates_Mcw_s": {}, "points": {}}
    g.synth_llr_dev(7, 0, Bmax, g.snr_sqrt_linear(2.0), llr.data_ptr(), info.data_ptr())
    same = True
    for B in BATCHES:
        rate = {v: [] for v in VARIANTS}
        for r in range(rounds + 1):                        # round 0 warms up
            for v in VARIANTS:
                g.set_mode(1 if v == "mode1" else 0)
                torch.cuda.synchronize()
                ev0.record()
                for _ in range(calls):
                    call(v, B)
                ev1.record()
                torch.cuda.synchronize()
                if r:
                    rate[v].append(calls * B / (ev0.elapsed_time(ev1) * 1e-3) / 1e6)
                if v == "mode1" and r == 0:
                    w = win[:B].long().clamp(min=0)
                    same = same and bool(torch.equal(cand[torch.arange(B, device="cuda"), w], out[:B])) and \
                        bool(torch.equal(pm[torch.arange(B, device="cuda"), w].view(torch.int64), dpm[:B].view(torch.int64)))
        res["rates_Mcw_s"][str(B)] = {v: summary(rate[v]) for v in VARIANTS}
    g.set_mode(0)
    B = BATCHES[0]
    for e in EBNO_POINTS:
        g.synth_llr_dev(11, 0, B, g.snr_sqrt_linear(e), llr.data_ptr(), info.data_ptr())
        call("list", B)
        g.list_find_dev(cand.data_ptr(), na.data_ptr(), info.data_ptr(), B, L, rank.data_ptr())
        torch.cuda.synchronize()
        rk, w = rank[:B], win[:B]
        res["points"]["%.1f" % e] = {"codewords": B, "list_miss": float((rk == L).float().mean()), "bler": float((rk != w).float().mean()),
                                     "sent_word_behind_row_0": float(((rk > 0) & (rk < L)).float().mean())}
    res["winner_row_equals_mode1_decode"] = same
    print("LIST " + json.dumps(res), flush=True)
    return 0 if same else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list", "rates.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--one")
    ap.add_argument("--configs", nargs="*", default=list(CONFIGS))
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.rounds, a.calls)
    from polar_amd import build
    build.build()
    results = {}
    for name in a.configs:
        # a fresh child per shape, ended by its own time limit; nothing further is started after a failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--rounds", str(a.rounds), "--calls", str(a.calls)],
                               capture_output=True, text=True, timeout=CONFIGS[name]["limit"])
        except subprocess.TimeoutExpired:
            print("list_rates: %s exceeded its time limit of %d s; stopping" % (name, CONFIGS[name]["limit"]), file=sys.stderr)
            return 124
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("LIST ")]
        if line:
            results[name] = json.loads(line[-1][5:])
            for B, row in results[name]["rates_Mcw_s"].items():
                print(name, "B", B, "  ".join("%s %.3f [%.3f - %.3f]" % (k, v["median"], v["min"], v["max"]) for k, v in row.items()), flush=True)
            print(name, "points", json.dumps(results[name]["points"]), flush=True)
        if r.returncode != 0:
            print("list_rates: %s failed (exit %d)\n%s" % (name, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return r.returncode
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump({"tool": "tools/list_rates.py", "rounds": a.rounds, "calls_per_round": a.calls,
               "clock": "HIP events around the back-to-back device-resident calls; M codewords / s",
               "results": results}, open(a.out, "w"), indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
