#!/usr/bin/env python3
"""tools/mlc_rates.py — rates of the multi-level coding (MLC) receiver (polar_kernels_mlc.hip) on one GPU, into a JSON file:

  * decode_mlc_dev (device-resident symbols and decisions): codewords/s from device events around the call (after a warm-up),
    ask4-sp and ask16-sp, N = 1024 / 2048, B = 1 / 64 / 4096 / 16384 / 65536, both geometries (lat_max_b forced: -1 = one lane per
    codeword, 1 << 30 = one codeword per wave);
  * in the same run, the host-pointer calls decode_mlc and decode_sc_p1 (PolarM's per-codeword decoder; it has no device entry
    point) at the same N and B, wall time per call, copies included on both sides;
  * end-to-end trials/s of main_MC_CC_Comparison.m's own MLC sweeps: design SNR + (-3:0.25:3), max_runs 100e3, max_err 250,
    codes from the shipped construction tables (tests/golden/construction_tables_mlc.npz).

The two decode_mlc_dev columns and the host-call columns are different clocks: compare decode_mlc with decode_sc_p1 (both host
calls), or compare KERNEL times. For those, run the tool under `rocprofv3 --kernel-trace --output-format csv -- python
tools/mlc_rates.py ...`: every decode call launches exactly one decoder kernel (mlc_sc_kernel, mlc_sc_lat_kernel, sc_p1_kernel or
sc_p1_lat_kernel), the output JSON lists the calls in launch order ("dispatch_log"), and
`python tools/mlc_rates.py --kernel-times <kernel_trace.csv> --calls <that JSON> --out <file>` pairs the two: median kernel
time per (call, constellation, N, B, geometry), for decode_mlc and decode_sc_p1 alike.

Sweeps: "loop_runs_per_s" is the reference loop's i_run iterations per second (max_runs / seconds; each iteration covers the whole
SNR grid: simulated at the first point it fails, counted at the others); "point_runs" is the sum of the run counters over the grid.

usage: python tools/mlc_rates.py [--out profiles/mlc/mlc_rates.json] [--quick]   (--quick: no sweeps, B <= 4096)
       python tools/mlc_rates.py --kernel-times TRACE.csv --calls RATES.json --out KERNEL_TIMES.json"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import polar_amd  # noqa: E402

DESIGN = {"ask4-sp": 4.5, "ask16-sp": 12.0}
TABLE = {"ask4-sp": "ask4-sp_4.5_250000", "ask16-sp": "ask16-sp_12_250000"}


DECODERS = ("mlc_sc_kernel", "mlc_sc_lat_kernel", "sc_p1_kernel", "sc_p1_lat_kernel")
CALLS = []          # one entry per decode call, in launch order (each launches one decoder kernel)


def _event_time(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / 1e3 / reps


def _wall_time(fn, reps):
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) / reps


def kernel_times(trace, calls_json, out):
    """Pair a rocprofv3 kernel trace of this tool's run with its dispatch log: median kernel time per call kind."""
    import csv
    import statistics
    rows = [r for r in csv.DictReader(open(trace)) if any(k + "(" in r["Kernel_Name"] for k in DECODERS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = json.load(open(calls_json))["dispatch_log"]
    if len(rows) < len(calls):
        raise SystemExit(f"{len(rows)} decoder dispatches in the trace, {len(calls)} decode calls in the log")
    rows = rows[: len(calls)]           # (the sweeps run after every decode call and add decoder dispatches of their own)
    acc = {}
    for r, c in zip(rows, calls):
        kname = next(k for k in DECODERS if k + "(" in r["Kernel_Name"])
        ent = acc.setdefault(tuple(c), {"kernel": kname, "ns": []})
        ent["ns"].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    res = [{"call": k[0], "const": k[1], "N": k[2], "B": k[3], "geometry": k[4], "kernel": v["kernel"], "calls": len(v["ns"]),
            "median_kernel_ms": statistics.median(v["ns"]) / 1e6, "kernel_cw_per_s": k[3] / (statistics.median(v["ns"]) / 1e9)}
           for k, v in acc.items()]
    with open(out, "w") as f:
        json.dump({"trace": os.path.basename(trace), "kernel_times": res}, f, indent=1)
    for r in res:
        print(json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlc", "mlc_rates.json"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--kernel-times", metavar="TRACE_CSV")
    ap.add_argument("--calls", metavar="RATES_JSON")
    a = ap.parse_args()
    if a.kernel_times:
        return kernel_times(a.kernel_times, a.calls, a.out)
    torch.cuda.set_device(0)
    Bs = (1, 64, 4096) if a.quick else (1, 64, 4096, 16384, 65536)
    rows = []
    for N in (1024, 2048):
        K = N // 2
        g = polar_amd.PolarCode.from_block_length(N, K, 0.32)
        rng = np.random.default_rng(N)
        p1_host = rng.random((max(Bs), N))
        for const in ("ask4-sp", "ask16-sp"):
            M = N // (2 if const == "ask4-sp" else 4)
            snr = DESIGN[const]
            n0 = 0.5 * 10 ** (-snr / 10)
            d_y = torch.empty((max(Bs), M), dtype=torch.float64, device="cuda")
            g.synth_mlc_dev(const, 1, 0, max(Bs), snr, d_y.data_ptr())
            y_host = d_y.cpu().numpy()
            for B in Bs:
                reps = 20 if B <= 64 else (5 if B <= 4096 else 2)
                out = torch.empty((B, K), dtype=torch.float64, device="cuda")
                for geo, lat in (("lane_per_codeword", -1), ("codeword_per_wave", 1 << 30)):
                    g.debug_set("lat_max_b", lat)
                    CALLS.extend([["decode_mlc_dev", const, N, B, geo]] * (reps + 1))
                    t = _event_time(lambda: g.decode_mlc_dev(const, d_y.data_ptr(), n0, B, out.data_ptr()), reps)
                    rows.append({"call": "decode_mlc_dev", "const": const, "N": N, "B": B, "geometry": geo, "s_per_call": t,
                                 "cw_per_s": B / t, "clock": "device events"})
                    print(json.dumps(rows[-1]), flush=True)
                g.debug_set("lat_max_b", 0)
                yb = np.ascontiguousarray(y_host[:B])
                CALLS.extend([["decode_mlc", const, N, B, "default"]] * (reps + 1))
                t = _wall_time(lambda: g.decode_mlc(yb, n0, const), reps)
                rows.append({"call": "decode_mlc", "const": const, "N": N, "B": B, "geometry": "default", "s_per_call": t,
                             "cw_per_s": B / t, "clock": "host wall, copies included"})
                print(json.dumps(rows[-1]), flush=True)
        for B in Bs:
            reps = 20 if B <= 64 else (5 if B <= 4096 else 2)
            pb = np.ascontiguousarray(p1_host[:B])
            CALLS.extend([["decode_sc_p1", None, N, B, "default"]] * (reps + 1))
            t = _wall_time(lambda: g.decode_sc_p1(pb), reps)
            rows.append({"call": "decode_sc_p1", "N": N, "B": B, "geometry": "default", "s_per_call": t, "cw_per_s": B / t,
                         "clock": "host wall, copies included"})
            print(json.dumps(rows[-1]), flush=True)
    sweeps = []
    if not a.quick:
        tabs = np.load(os.path.join(ROOT, "tests", "golden", "construction_tables_mlc.npz"))
        for const in ("ask4-sp", "ask16-sp"):
            g = polar_amd.PolarCode.from_counts(tabs[TABLE[const] + "/counts"].astype(np.int64), 512)
            axis = DESIGN[const] + np.arange(-3, 3.001, 0.25)
            g.get_bler_quick(axis[:2], [1], max_runs=2000, max_err=250, constellation=const, receiver="mlc")   # warm-up
            t = time.perf_counter()
            bler, c = g.get_bler_quick(axis, [1], max_runs=100000, max_err=250, constellation=const, receiver="mlc",
                                       return_counters=True)
            dt = time.perf_counter() - t
            run = c["run"][0].astype(np.int64)
            sweeps.append({"const": const, "axis": axis.tolist(), "bler": bler[0].tolist(), "run": run.tolist(),
                           "err": c["err"][0].astype(np.int64).tolist(), "seconds": dt, "rounds": c["rounds"],
                           "loop_runs": 100000, "loop_runs_per_s": 100000 / dt, "point_runs": int(run.sum())})
            print(json.dumps({k: v for k, v in sweeps[-1].items() if k in ("const", "seconds", "loop_runs_per_s", "point_runs", "rounds")}),
                  flush=True)
    res = {"device": torch.cuda.get_device_name(0), "decode": rows, "sweeps": sweeps, "dispatch_log": CALLS}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
