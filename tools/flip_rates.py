"""Rate and BLER of SC-Flip (decode_sc_flip_dev) beside the fixed small lists and the adaptive schedule -> profiles/flip/rates.json
(DESIGN.md §8h).

Device-resident, synthetic workload: the headline code N = 2048, K = 1024, CRC 16 at Eb/N0 1.5, 2.0 and 2.5 dB, B = 8 192 and 65 536.
Variants on the same rows, alternated inside one process:
  flip0, flip8, flip32   decode_sc_flip_dev with max_flips 0, 8, 32, every output but the candidates;
  L1, L2, L4, L8         decode_scl_llr_dev at that list size under polar_set_mode(1), batch kernels (no one-codeword-per-wave form);
  1-4-32                 decode_scl_llr_adaptive_dev with that schedule.
One warm-up round, `--rounds` timed rounds of `--calls` back-to-back calls between HIP events; median [min - max] in M codewords / s.
Per variant also the block errors against the sent words on those rows; per SC-Flip variant the first-pass, flipped and failed shares
and the mean number of SC passes. Beside it the BLER of flip_stats at the three max_flips and of list_stats at L = 1, 2, 4, 8 on the
same points (`--max-runs` trials, `--max-err` errors).
Each Eb/N0 point runs in a child process of its own under a time limit; a failed child ends the run.

    python tools/flip_rates.py [--out profiles/flip/rates.json] [--rounds 3] [--calls 2]
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
BATCHES = (8192, 65536)
FLIPS = (0, 8, 32)
LISTS = (1, 2, 4, 8)
SCHEDULE = (1, 4, 32)
LIMIT = 400          # seconds per Eb/N0 point


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": xs}


def one(ebno, rounds, calls, max_runs, max_err):
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
    nd = torch.zeros(Bmax, dtype=torch.uint8, device="cuda")
    flip = torch.zeros(Bmax, dtype=torch.int32, device="cuda")
    g.debug_set("lat_max_b", -1)
    variants = ["flip%d" % t for t in FLIPS] + ["L%d" % L for L in LISTS] + ["-".join(str(x) for x in SCHEDULE)]

    def call(v, B):
        if v.startswith("flip"):
            g.decode_sc_flip_dev(llr.data_ptr(), "f64", B, int(v[4:]), out.data_ptr(), ok.data_ptr(), nd.data_ptr(), flip.data_ptr())
        elif v.startswith("L"):
            g.decode_scl_llr_dev(llr.data_ptr(), B, int(v[1:]), out.data_ptr(), pm.data_ptr())
        else:
            g.decode_scl_llr_adaptive_dev(llr.data_ptr(), "f64", B, SCHEDULE, out.data_ptr(), pm.data_ptr(), stage.data_ptr(), ok.data_ptr())

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {"ebno_db": ebno, "rates_Mcw_s": {}, "rows": {}}
    g.synth_llr_dev(7, 0, Bmax, g.snr_sqrt_linear(ebno), llr.data_ptr(), info.data_ptr())
    for B in BATCHES:
        rate = {v: [] for v in variants}
        rows = {}
        for r in range(rounds + 1):                        # round 0 warms up
            for v in variants:
                g.set_mode(1 if v.startswith("L") else 0)
                torch.cuda.synchronize()
                ev0.record()
                for _ in range(calls):
                    call(v, B)
                ev1.record()
                torch.cuda.synchronize()
                if r:
                    rate[v].append(calls * B / (ev0.elapsed_time(ev1) * 1e-3) / 1e6)
                else:
                    row = {"block_errors": int((out[:B] != info[:B]).any(dim=1).sum())}
                    if v.startswith("flip"):
                        okb, ndb = ok[:B] == 1, nd[:B].long()
                        row["first_share"] = float((okb & (ndb == 1)).sum()) / B
                        row["flipped_share"] = float((okb & (ndb > 1)).sum()) / B
                        row["failed_share"] = float((~okb).sum()) / B
                        row["mean_decodes"] = float(ndb.sum()) / B
                    rows[v] = row
        g.set_mode(0)
        res["rates_Mcw_s"][str(B)] = {k: summary(x) for k, x in rate.items()}
        res["rows"][str(B)] = rows
    # BLER on the sweep's own trials: SC-Flip beside the fixed lists
    bler = {}
    for t in FLIPS:
        s = g.flip_stats([ebno], t, max_runs=max_runs, max_err=max_err, seed=11)
        bler["flip%d" % t] = {"bler": float(s["bler"][0]), "undetected_rate": float(s["undetected_rate"][0]),
                              "mean_decodes": float(s["mean_decodes"][0]), "runs": int(s["stats"][0, polar_amd.FL_RUN]),
                              "errors": int(s["stats"][0, polar_amd.FL_ERR])}
    ls = g.list_stats([ebno], list(LISTS), max_runs=max_runs, max_err=max_err, seed=11)
    for i, L in enumerate(LISTS):
        bler["L%d" % L] = {"bler": float(ls["bler"][i, 0]), "undetected_rate": float(ls["undetected_rate"][i, 0]),
                           "runs": int(ls["stats"][i, 0, polar_amd.LS_RUN]), "errors": int(ls["stats"][i, 0, polar_amd.LS_ERR])}
    res["bler"] = bler
    print("FLIP " + json.dumps(res), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flip", "rates.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--max-runs", type=int, default=200000)
    ap.add_argument("--max-err", type=int, default=200)
    ap.add_argument("--one", type=float)
    ap.add_argument("--points", nargs="*", type=float, default=list(EBNO_POINTS))
    a = ap.parse_args()
    if a.one is not None:
        return one(a.one, a.rounds, a.calls, a.max_runs, a.max_err)
    from polar_amd import build
    build.build()
    results = {}
    for e in a.points:
        # a fresh child per point, ended by its own time limit; nothing further is started after a failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(e), "--rounds", str(a.rounds), "--calls", str(a.calls),
                                "--max-runs", str(a.max_runs), "--max-err", str(a.max_err)], capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            print("flip_rates: %.1f dB exceeded its time limit of %d s; stopping" % (e, LIMIT), file=sys.stderr)
            return 124
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("FLIP ")]
        if line:
            res = results["%.1f" % e] = json.loads(line[-1][5:])
            for B, row in res["rates_Mcw_s"].items():
                print("%.1f dB B %s " % (e, B) + "  ".join("%s %.3f [%.3f - %.3f]" % (k, v["median"], v["min"], v["max"]) for k, v in row.items()), flush=True)
                print("%.1f dB B %s rows " % (e, B) + json.dumps(res["rows"][B]), flush=True)
            print("%.1f dB bler " % e + json.dumps(res["bler"]), flush=True)
        if r.returncode != 0:
            print("flip_rates: %.1f dB failed (exit %d)\n%s" % (e, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return r.returncode
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump({"tool": "tools/flip_rates.py", "code": CODE, "rounds": a.rounds, "calls_per_round": a.calls,
               "clock": "HIP events around the back-to-back device-resident calls; M codewords / s",
               "bler_stop": {"max_runs": a.max_runs, "max_err": a.max_err}, "results": results}, open(a.out, "w"), indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
