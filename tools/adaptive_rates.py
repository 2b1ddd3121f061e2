"""Rate of the adaptive list decode (decode_scl_llr_adaptive_dev) beside the fixed list of 32 -> profiles/adaptive/rates.json
(DESIGN.md §8g).

Device-resident, synthetic workload: the headline code N = 2048, K = 1024, CRC 16 at Eb/N0 1.5, 2.0 and 2.5 dB, B = 65 536 and 8 192.
Five variants on the same rows, alternated inside one process:
  1-4-32, 1-2-4-8-16-32, 4-32   decode_scl_llr_adaptive_dev with that schedule, all four outputs;
  mode1                         decode_scl_llr_dev at L = 32 under polar_set_mode(1), batch kernel: the same arithmetic, the fair parent;
  auto                          decode_scl_llr_dev at L = 32 under automatic mode (the headline kernel).
One warm-up round, `--rounds` timed rounds of `--calls` back-to-back calls between HIP events; median [min - max] in M codewords / s.
Per variant also the block errors against the sent words on those rows, and per schedule the share of the codewords each stage
delivered and the mean effort (the list sizes a codeword went through; the fixed list costs 32).
Each Eb/N0 point runs in a child process of its own under a time limit; a failed child ends the run.

    python tools/adaptive_rates.py [--out profiles/adaptive/rates.json] [--rounds 3] [--calls 2]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CODE = dict(n=11, K=1024, crc=16)
EBNO_POINTS = (1.5, 2.0, 2.5)
BATCHES = (65536, 8192)
SCHEDULES = ((1, 4, 32), (1, 2, 4, 8, 16, 32), (4, 32))
FIXED_L = 32
LIMIT = 400          # seconds per Eb/N0 point


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": xs}


def name_of(v):
    return v if isinstance(v, str) else "-".join(str(x) for x in v)


def one(ebno, rounds, calls):
    import ctypes as C
    import numpy as np
    import torch
    import polar_amd
    n, K = CODE["n"], CODE["K"]
    N = 1 << n
    torch.cuda.set_device(0)
    C.CDLL(None).srand(C.c_uint(1))
    g = polar_amd.PolarCode(n, K, 0.32, CODE["crc"])
    Bmax = max(BATCHES)
    llr = torch.empty((Bmax, N), dtype=torch.float64, device="cuda")
    info = torch.empty((Bmax, K), dtype=torch.uint8, device="cuda")
    out = torch.zeros((Bmax, K), dtype=torch.uint8, device="cuda")
    pm = torch.zeros(Bmax, dtype=torch.float64, device="cuda")
    stage = torch.zeros(Bmax, dtype=torch.uint8, device="cuda")
    ok = torch.zeros(Bmax, dtype=torch.uint8, device="cuda")
    g.debug_set("lat_max_b", -1)
    variants = list(SCHEDULES) + ["mode1", "auto"]

    def call(v, B):
        if isinstance(v, tuple):
            g.decode_scl_llr_adaptive_dev(llr.data_ptr(), "f64", B, v, out.data_ptr(), pm.data_ptr(), stage.data_ptr(), ok.data_ptr())
        else:
            g.decode_scl_llr_dev(llr.data_ptr(), B, FIXED_L, out.data_ptr(), pm.data_ptr())

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {"ebno_db": ebno, "rates_Mcw_s": {}, "rows": {}}
    g.synth_llr_dev(7, 0, Bmax, g.snr_sqrt_linear(ebno), llr.data_ptr(), info.data_ptr())
    for B in BATCHES:
        rate = {name_of(v): [] for v in variants}
        rows = {}
        for r in range(rounds + 1):                        # round 0 warms up
            for v in variants:
                g.set_mode(1 if v == "mode1" else 0)
                torch.cuda.synchronize()
                ev0.record()
                for _ in range(calls):
                    call(v, B)
                ev1.record()
                torch.cuda.synchronize()
                if r:
                    rate[name_of(v)].append(calls * B / (ev0.elapsed_time(ev1) * 1e-3) / 1e6)
                else:
                    row = {"block_errors": int((out[:B] != info[:B]).any(dim=1).sum())}
                    if isinstance(v, tuple):
                        cnt = torch.bincount(stage[:B].long(), minlength=len(v)).cpu().numpy()
                        row["stage_share"] = (cnt / B).tolist()
                        row["mean_effort"] = float((cnt / B) @ np.cumsum(np.array(v, np.float64)))
                        row["accepted"] = int(ok[:B].sum())
                    rows[name_of(v)] = row
        g.set_mode(0)
        res["rates_Mcw_s"][str(B)] = {k: summary(x) for k, x in rate.items()}
        res["rows"][str(B)] = rows
    print("ADAPT " + json.dumps(res), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive", "rates.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--one", type=float)
    ap.add_argument("--points", nargs="*", type=float, default=list(EBNO_POINTS))
    a = ap.parse_args()
    if a.one is not None:
        return one(a.one, a.rounds, a.calls)
    from polar_amd import build
    build.build()
    results = {}
    for e in a.points:
        # a fresh child per point, ended by its own time limit; nothing further is started after a failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(e), "--rounds", str(a.rounds), "--calls", str(a.calls)],
                               capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            print("adaptive_rates: %.1f dB exceeded its time limit of %d s; stopping" % (e, LIMIT), file=sys.stderr)
            return 124
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("ADAPT ")]
        if line:
            res = results["%.1f" % e] = json.loads(line[-1][6:])
            for B, row in res["rates_Mcw_s"].items():
                print("%.1f dB B %s " % (e, B) + "  ".join("%s %.3f [%.3f - %.3f]" % (k, v["median"], v["min"], v["max"]) for k, v in row.items()), flush=True)
                print("%.1f dB B %s rows " % (e, B) + json.dumps(res["rows"][B]), flush=True)
        if r.returncode != 0:
            print("adaptive_rates: %.1f dB failed (exit %d)\n%s" % (e, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return r.returncode
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump({"tool": "tools/adaptive_rates.py", "code": CODE, "rounds": a.rounds, "calls_per_round": a.calls,
               "clock": "HIP events around the back-to-back device-resident calls; M codewords / s",
               "results": results}, open(a.out, "w"), indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
