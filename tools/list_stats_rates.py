"""What the error analysis of the list decoder costs on top of the decode it analyses -> profiles/list/stats.json.

Synthetic BPSK workload at Eb/N0 2 dB, T = 8 192 trials per call. Shapes: N = 2048, K = 1024, CRC 16 at L = 32; N = 1024, K = 512,
CRC 8 at L = 8 and at L = 1. Two variants, alternated inside one process:
  stats       polar_mc_batch_list (one point): synth, list decode, the sent word's metric, classification, counters read back;
  baseline    the same trials through synth_llr_dev + decode_scl_llr_list_dev alone and a device synchronise — both calls exist
              without the error analysis, so this is what it is added to.
One warm-up round, `--rounds` timed rounds of `--calls` calls under a host clock (each variant ends in a synchronisation);
median [min - max] in k trials / s. share_added = 1 - stats / baseline: the metric kernel, the classification and the read-back.
Each shape runs in a child process of its own under a time limit; a failed child ends the run.

    python tools/list_stats_rates.py [--out profiles/list/stats.json] [--rounds 3] [--calls 2]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "headline_l32": dict(n=11, K=1024, crc=16, L=32, limit=300),
    "n1024_l8": dict(n=10, K=512, crc=8, L=8, limit=180),
    "n1024_l1": dict(n=10, K=512, crc=8, L=1, limit=180),
}
T = 8192
EBNO = 2.0
VARIANTS = ("stats", "baseline")


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": xs}


def one(name, rounds, calls):
    import ctypes as C
    import numpy as np
    import torch
    import polar_amd
    c = CONFIGS[name]
    n, K, crc, L = c["n"], c["K"], c["crc"], c["L"]
    N = 1 << n
    torch.cuda.set_device(0)
    C.CDLL(None).srand(C.c_uint(1))
    g = polar_amd.PolarCode(n, K, 0.32, crc)
    llr = torch.empty((T, N), dtype=torch.float64, device="cuda")
    info = torch.empty((T, K), dtype=torch.uint8, device="cuda")
    cand = torch.zeros((T, L, K), dtype=torch.uint8, device="cuda")
    pm = torch.zeros((T, L), dtype=torch.float64, device="cuda")
    ok = torch.zeros((T, L), dtype=torch.uint8, device="cuda")
    na = torch.zeros(T, dtype=torch.int32, device="cuda")
    win = torch.zeros(T, dtype=torch.int32, device="cuda")
    stats = np.zeros((1, 1, polar_amd.LS_N), np.uint64)
    en = np.ones((1, 1), np.uint8)

    def call(v):
        if v == "stats":
            g.mc_batch_list(7, 0, T, 1, [EBNO], [L], en, stats)
        else:
            g.synth_llr_dev(7, 0, T, g.snr_sqrt_linear(EBNO), llr.data_ptr(), info.data_ptr())
            g.decode_scl_llr_list_dev(llr.data_ptr(), "f64", T, L, cand.data_ptr(), pm.data_ptr(), ok.data_ptr(), na.data_ptr(), win.data_ptr())
            torch.cuda.synchronize()

    rate = {v: [] for v in VARIANTS}
    for r in range(rounds + 1):                        # round 0 warms up
        for v in VARIANTS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                call(v)
            dt = time.perf_counter() - t0
            if r:
                rate[v].append(calls * T / dt / 1e3)
    # the baseline's own rows say what the counters must be: winner row against the sent info
    w = win.long().clamp(min=0)
    err = int((cand[torch.arange(T, device="cuda"), w] != info).any(dim=1).sum())
    per_call = stats[0, 0] // np.uint64((rounds + 1) * calls)
    same = int(per_call[polar_amd.LS_ERR]) == err and int(per_call[polar_amd.LS_RUN]) == T
    res = {"config": {k: c[k] for k in ("n", "K", "crc", "L")}, "trials_per_call": T, "ebno_db": EBNO,
           "rates_ktrials_s": {v: summary(rate[v]) for v in VARIANTS},
           "share_added": 1.0 - statistics.median(rate["stats"]) / statistics.median(rate["baseline"]),
           "counters_per_call": [int(x) for x in per_call], "err_equals_baseline_rows": same}
    print("STATS " + json.dumps(res), flush=True)
    return 0 if same else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list", "stats.json"))
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
            print("list_stats_rates: %s exceeded its time limit of %d s; stopping" % (name, CONFIGS[name]["limit"]), file=sys.stderr)
            return 124
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("STATS ")]
        if line:
            results[name] = json.loads(line[-1][6:])
            print(name, "  ".join("%s %.1f [%.1f - %.1f]" % (k, v["median"], v["min"], v["max"]) for k, v in results[name]["rates_ktrials_s"].items()),
                  "share added %.3f" % results[name]["share_added"], "counters", results[name]["counters_per_call"], flush=True)
        if r.returncode != 0:
            print("list_stats_rates: %s failed (exit %d)\n%s" % (name, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return r.returncode
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump({"tool": "tools/list_stats_rates.py", "rounds": a.rounds, "calls_per_round": a.calls,
               "clock": "host clock around calls that end in a device synchronisation; k trials / s",
               "results": results}, open(a.out, "w"), indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
