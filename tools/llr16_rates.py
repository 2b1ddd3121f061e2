"""Decode rates by element format of the channel LLRs (f64 / f32 / f16 / bf16) -> profiles/llr16/rates.json.

Configurations: N = 2048, K = 1024, L = 1 at B = 65 536 and 262 144; the headline N = 2048, K = 1024, CRC 16, L = 32 at
B = 65 536. The four variants hold the SAME values (the synthetic rows rounded to what both 16-bit formats represent), are
alternated inside one process, and must give the same bits. Per variant: one warm-up round, five timed rounds, median [min - max].
Two clocks, reported in separate columns and not to be compared with each other:
  dev_Mcw_s   device-resident rows, HIP events around `--calls` back-to-back calls;
  host_Mcw_s  host-pointer call (pageable numpy rows in, bits out), wall clock around the call.
Each configuration runs in a child process of its own under a time limit; a failed child ends the run.

    python tools/llr16_rates.py [--out profiles/llr16/rates.json] [--rounds 5] [--calls 3]
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
    "l1_b65536": dict(n=11, K=1024, crc=0, L=1, B=65536, limit=240),
    "l1_b262144": dict(n=11, K=1024, crc=0, L=1, B=262144, limit=420),
    "headline_l32_b65536": dict(n=11, K=1024, crc=16, L=32, B=65536, limit=420),
}
VARIANTS = ("f64", "f32", "f16", "bf16")


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": xs}


def one(name, rounds, calls):
    import ctypes as C
    import numpy as np
    import torch
    import polar_amd
    c = CONFIGS[name]
    n, K, crc, L, B = c["n"], c["K"], c["crc"], c["L"], c["B"]
    N = 1 << n
    torch.cuda.set_device(0)
    C.CDLL(None).srand(C.c_uint(1))
    g = polar_amd.PolarCode(n, K, 0.32, crc)
    raw = torch.empty((B, N), dtype=torch.float64, device="cuda")
    g.synth_llr_dev(7, 0, B, g.snr_sqrt_linear(2.0), raw.data_ptr())
    # values both 16-bit formats hold exactly: bfloat16's 8 significant bits inside binary16's range
    v16 = raw.to(torch.bfloat16).to(torch.float16)
    dev = {"f64": v16.to(torch.float64), "f32": v16.to(torch.float32), "f16": v16, "bf16": v16.to(torch.bfloat16)}
    del raw
    same = all(bool(torch.equal(dev[k].to(torch.float64), dev["f64"])) for k in VARIANTS)
    host = {"f64": dev["f64"].cpu().numpy(), "f32": dev["f32"].cpu().numpy(), "f16": dev["f16"].cpu().numpy(),
            "bf16": dev["bf16"].view(torch.int16).cpu().numpy().view(np.uint16)}
    g.reserve(B, L)
    d_out = {k: torch.zeros((B, K), dtype=torch.uint8, device="cuda") for k in VARIANTS}
    h_out = {k: np.zeros((B, K), np.uint8) for k in VARIANTS}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_rate = {k: [] for k in VARIANTS}
    host_rate = {k: [] for k in VARIANTS}
    for r in range(rounds + 1):                        # round 0 warms up
        for k in VARIANTS:
            torch.cuda.synchronize()
            ev0.record()
            for _ in range(calls):
                g.decode_scl_llr_dev_fmt(dev[k].data_ptr(), k, B, L, d_out[k].data_ptr())
            ev1.record()
            torch.cuda.synchronize()
            if r:
                dev_rate[k].append(calls * B / (ev0.elapsed_time(ev1) * 1e-3) / 1e6)
        for k in VARIANTS:
            t0 = time.perf_counter()
            g.decode_scl_llr(host[k], L, out=h_out[k], fmt=k)
            dt = time.perf_counter() - t0
            if r:
                host_rate[k].append(B / dt / 1e6)
    ref = d_out["f64"].cpu().numpy()
    bits_equal = all((d_out[k].cpu().numpy() == ref).all() and (h_out[k] == ref).all() for k in VARIANTS)
    res = {"config": {k: c[k] for k in ("n", "K", "crc", "L", "B")}, "same_values_in_all_variants": same, "bits_equal": bool(bits_equal),
           "host_chunks_last_call": g.debug_get("host_chunks"),
           "bytes_per_codeword": {"f64": 8 * N, "f32": 4 * N, "f16": 2 * N, "bf16": 2 * N},
           "dev_Mcw_s": {k: summary(dev_rate[k]) for k in VARIANTS}, "host_Mcw_s": {k: summary(host_rate[k]) for k in VARIANTS}}
    print("LLR16 " + json.dumps(res), flush=True)
    return 0 if (same and bits_equal) else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "llr16", "rates.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--one")
    ap.add_argument("--configs", nargs="*", default=list(CONFIGS))
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.rounds, a.calls)
    from polar_amd import build
    build.build()
    results = {}
    for name in a.configs:
        # a fresh child per configuration, ended by its own time limit; nothing further is started after a failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--rounds", str(a.rounds), "--calls", str(a.calls)],
                               capture_output=True, text=True, timeout=CONFIGS[name]["limit"])
        except subprocess.TimeoutExpired:
            print("llr16_rates: %s exceeded its time limit of %d s; stopping" % (name, CONFIGS[name]["limit"]), file=sys.stderr)
            return 124
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("LLR16 ")]
        if line:
            results[name] = json.loads(line[-1][6:])
            for col in ("dev_Mcw_s", "host_Mcw_s"):
                print(name, col, "  ".join("%s %.2f [%.2f - %.2f]" % (k, v["median"], v["min"], v["max"]) for k, v in results[name][col].items()), flush=True)
        if r.returncode != 0:
            print("llr16_rates: %s failed (exit %d)\n%s" % (name, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return r.returncode
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump({"tool": "tools/llr16_rates.py", "rounds": a.rounds, "calls_per_device_round": a.calls,
               "clocks": {"dev_Mcw_s": "HIP events around the back-to-back device-resident calls",
                          "host_Mcw_s": "wall clock around one host-pointer call; not comparable with dev_Mcw_s"},
               "results": results}, open(a.out, "w"), indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
