"""Rate and BLER of SCAN soft-output decoding (decode_scan_dev) beside SC-Flip without retries and the list of 1 -> profiles/scan/rates.json
(DESIGN.md §8i).

Device-resident, synthetic workload: the headline code N = 2048, K = 1024, CRC 16 and N = 1024, K = 512, CRC 8, rows at Eb/N0 2.0 dB,
B = 8 192 and 65 536. Variants on the same rows, alternated inside one process:
  scan<i>[m][e]          decode_scan_dev with i = 1, 2, 4 iterations, every output; m: min-sum arithmetic, e: early stop;
  flip0                  decode_sc_flip_dev with max_flips = 0 — the same mapping (one codeword per wave, state in LDS), hard output;
  L1                     decode_scl_llr_dev at list size 1 under polar_set_mode(1), batch kernels.
One warm-up round, `--rounds` timed rounds of `--calls` back-to-back calls between HIP events; median [min - max] in M codewords / s.
Per variant also the block errors against the sent words on those rows and, for SCAN, the mean number of iterations. Beside it the
BLER of scan_stats at 1, 2, 4 iterations (exact arithmetic, no early stop: it changes no decision of a word that passes) and of
flip_stats(max_flips = 0) on the same trials at 1.5, 2.0 and 2.5 dB (`--max-runs` trials, `--max-err` errors).
Each code runs in a child process of its own under a time limit; a failed child ends the run.

    python tools/scan_rates.py [--out profiles/scan/rates.json] [--rounds 3] [--calls 2]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CODES = ((11, 1024, 16), (10, 512, 8))
RATE_EBNO = 2.0
EBNO_POINTS = (1.5, 2.0, 2.5)
BATCHES = (8192, 65536)
ITERS = (1, 2, 4)
LIMIT = 500          # seconds per code


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": xs}


def one(code, rounds, calls, max_runs, max_err):
    import ctypes as C
    import torch
    import polar_amd
    n, K, crc = code
    N = 1 << n
    torch.cuda.set_device(0)
    C.CDLL(None).srand(C.c_uint(1))
    g = polar_amd.PolarCode(n, K, 0.32, crc)
    Bmax = max(BATCHES)
    llr = torch.empty((Bmax, N), dtype=torch.float64, device="cuda")
    info = torch.empty((Bmax, K), dtype=torch.uint8, device="cuda")
    out = torch.zeros((Bmax, K), dtype=torch.uint8, device="cuda")
    soft = torch.zeros((Bmax, K), dtype=torch.float64, device="cuda")
    ext = torch.zeros((Bmax, N), dtype=torch.float64, device="cuda")
    pm = torch.zeros(Bmax, dtype=torch.float64, device="cuda")
    ok = torch.zeros(Bmax, dtype=torch.uint8, device="cuda")
    nit = torch.zeros(Bmax, dtype=torch.uint8, device="cuda")
    flip = torch.zeros(Bmax, dtype=torch.int32, device="cuda")
    g.debug_set("lat_max_b", -1)
    variants = ["scan%d%s%s" % (i, m, e) for i in ITERS for m in ("", "m") for e in ("", "e")] + ["flip0", "L1"]

    def call(v, B):
        if v.startswith("scan"):
            g.decode_scan_dev(llr.data_ptr(), "f64", B, int(v[4]), out.data_ptr(), soft.data_ptr(), ext.data_ptr(), ok.data_ptr(),
                              nit.data_ptr(), minsum="m" in v[5:], early_stop="e" in v[5:])
        elif v == "flip0":
            g.decode_sc_flip_dev(llr.data_ptr(), "f64", B, 0, out.data_ptr(), ok.data_ptr(), nit.data_ptr(), flip.data_ptr())
        else:
            g.decode_scl_llr_dev(llr.data_ptr(), B, 1, out.data_ptr(), pm.data_ptr())

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {"code": list(code), "rate_ebno_db": RATE_EBNO, "rates_Mcw_s": {}, "rows": {}}
    g.synth_llr_dev(7, 0, Bmax, g.snr_sqrt_linear(RATE_EBNO), llr.data_ptr(), info.data_ptr())
    for B in BATCHES:
        rate = {v: [] for v in variants}
        rows = {}
        for r in range(rounds + 1):                        # round 0 warms up
            for v in variants:
                g.set_mode(1 if v == "L1" else 0)
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
                    if v.startswith("scan"):
                        row["mean_iters"] = float(nit[:B].long().sum()) / B
                        row["crc_ok_share"] = float((ok[:B] == 1).sum()) / B
                    rows[v] = row
        g.set_mode(0)
        res["rates_Mcw_s"][str(B)] = {k: summary(x) for k, x in rate.items()}
        res["rows"][str(B)] = rows
    # BLER on the sweep's own trials: SCAN beside SC without retries
    bler = {}
    pts = list(EBNO_POINTS)
    for i in ITERS:
        s = g.scan_stats(pts, i, max_runs=max_runs, max_err=max_err, seed=11)
        bler["scan%d" % i] = {"bler": s["bler"].tolist(), "undetected_rate": s["undetected_rate"].tolist(),
                              "runs": s["stats"][:, polar_amd.SN_RUN].tolist(), "errors": s["stats"][:, polar_amd.SN_ERR].tolist()}
    s = g.flip_stats(pts, 0, max_runs=max_runs, max_err=max_err, seed=11)
    bler["flip0"] = {"bler": s["bler"].tolist(), "undetected_rate": s["undetected_rate"].tolist(),
                     "runs": s["stats"][:, polar_amd.FL_RUN].tolist(), "errors": s["stats"][:, polar_amd.FL_ERR].tolist()}
    res["bler_ebno_db"] = pts
    res["bler"] = bler
    print("SCAN " + json.dumps(res), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan", "rates.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--max-runs", type=int, default=100000)
    ap.add_argument("--max-err", type=int, default=200)
    ap.add_argument("--one", type=int, help="index into CODES (a child of this tool)")
    a = ap.parse_args()
    if a.one is not None:
        return one(CODES[a.one], a.rounds, a.calls, a.max_runs, a.max_err)
    from polar_amd import build
    build.build()
    results = {}
    for k, code in enumerate(CODES):
        # a fresh child per code, ended by its own time limit; nothing further is started after a failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(k), "--rounds", str(a.rounds), "--calls", str(a.calls),
                                "--max-runs", str(a.max_runs), "--max-err", str(a.max_err)], capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            print("scan_rates: %r exceeded its time limit of %d s; stopping" % (code, LIMIT), file=sys.stderr)
            return 124
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("SCAN ")]
        if line:
            res = results["%d,%d,%d" % code] = json.loads(line[-1][5:])
            for B, row in res["rates_Mcw_s"].items():
                print("%r B %s " % (code, B) + "  ".join("%s %.3f [%.3f - %.3f]" % (k2, v["median"], v["min"], v["max"]) for k2, v in row.items()), flush=True)
                print("%r B %s rows " % (code, B) + json.dumps(res["rows"][B]), flush=True)
            print("%r bler " % (code,) + json.dumps(res["bler"]), flush=True)
        if r.returncode != 0:
            print("scan_rates: %r failed (exit %d)\n%s" % (code, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return r.returncode
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump({"tool": "tools/scan_rates.py", "rounds": a.rounds, "calls_per_round": a.calls,
               "clock": "HIP events around the back-to-back device-resident calls; M codewords / s",
               "bler_stop": {"max_runs": a.max_runs, "max_err": a.max_err}, "results": results}, open(a.out, "w"), indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
