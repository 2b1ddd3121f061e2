#!/usr/bin/env python3
"""tools/bicm_rx_rates.py — what decoding from received symbols costs or saves against decoding from ready LLRs, on one GPU,
into profiles/bicm_rx/rates.json (quoted in DESIGN.md §8c).

Workloads: configuration 5 (the cfg5_n10_k512_ask16 tables, N = 1024, 16-ASK Gray) at L = 1 and L = 8, and the headline shape
(N = 2048, K = 1024, 16-bit CRC) with 4-ASK Gray at L = 32; batches of 65 536 and 262 144 codewords.

Variants, alternated within one process, one warm-up round and then `--reps` (>= 5) timed rounds, median / min / max:
  (a) decode_scl_llr on ready host LLR doubles — the caller's own demapping is NOT in the time, which favours this variant;
  (b) decode_bicm on float64 symbols;  (c) decode_bicm on float32 symbols      [host wall clock around calls that return bits]
  (d) decode_scl_llr_dev against decode_bicm_dev on device-resident inputs, and the demap kernel alone (compute_llr_bicm_dev)
                                                                               [device events around the calls]
"criteria" evaluates the two comparisons the design rests on, from these numbers alone:
  copy-bound shape (cfg5, L = 1, 262 144, host pointers): slowest (b) repetition faster than the fastest (a) repetition;
  device-bound shapes (L = 8, L = 32, device pointers): median(bicm_dev) - median(llr_dev) <= (max - min)(llr_dev) + demap time.

usage: python tools/bicm_rx_rates.py [--out profiles/bicm_rx/rates.json] [--reps 5] [--quick]   (--quick: 8192 codewords only)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import polar_amd  # noqa: E402


def _stats(ts, B):
    med = statistics.median(ts)
    return {"median_s": med, "min_s": min(ts), "max_s": max(ts), "reps": len(ts), "median_cw_per_s": B / med}


def _wall(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def _event(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / 1e3


def _alternate(variants, reps):
    """variants: name -> (timer, fn). One untimed round, then `reps` rounds in which the variants take turns."""
    for _, fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(reps):
        for k, (timer, fn) in variants.items():
            ts[k].append(timer(fn))
    return ts


def measure(name, g, const, snr, L, B, reps):
    con = polar_amd.Constellation(const)
    n0 = 0.5 * 10 ** (-snr / 10)
    N, K, M = g.N, g.K, g.N // con.n_bits
    d_y = torch.empty((B, M), dtype=torch.float64, device="cuda")
    d_llr = torch.empty((B, N), dtype=torch.float64, device="cuda")
    g.synth_bicm_sym_dev(const, 1, 0, B, snr, d_y.data_ptr())
    con.compute_llr_bicm_dev(d_y.data_ptr(), N, B, n0, d_llr.data_ptr())
    torch.cuda.synchronize()
    y, y32, llr = d_y.cpu().numpy(), d_y.to(torch.float32).cpu().numpy(), d_llr.cpu().numpy()
    out_a, out_b, out_c = (np.zeros((B, K), np.uint8) for _ in range(3))
    host = _alternate({
        "a_decode_scl_llr_f64_llr": (_wall, lambda: g.decode_scl_llr(llr, L, out=out_a)),
        "b_decode_bicm_f64_sym": (_wall, lambda: g.decode_bicm(y, n0, con, L, out=out_b)),
        "c_decode_bicm_f32_sym": (_wall, lambda: g.decode_bicm(y32, n0, con, L, out=out_c)),
    }, reps)
    chunks = g.debug_get("host_chunks")
    bits_equal = bool((out_a == out_b).all())
    d_o1 = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    d_o2 = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    d_scratch = torch.empty((B, N), dtype=torch.float64, device="cuda")
    dev = _alternate({
        "d_decode_scl_llr_dev": (_event, lambda: g.decode_scl_llr_dev(d_llr.data_ptr(), B, L, d_o1.data_ptr())),
        "d_decode_bicm_dev": (_event, lambda: g.decode_bicm_dev(con, d_y.data_ptr(), n0, B, L, d_o2.data_ptr())),
        "d_demap_kernel_alone": (_event, lambda: con.compute_llr_bicm_dev(d_y.data_ptr(), N, B, n0, d_scratch.data_ptr())),
    }, reps)
    bits_equal = bits_equal and bool(torch.equal(d_o1, d_o2)) and bool((d_o1.cpu().numpy() == out_b).all())
    row = {"workload": name, "constellation": const, "N": N, "K": K, "crc": g.crc_size, "L": L, "B": B, "snr_db": snr,
           "input_bytes": {"llr_f64": B * N * 8, "sym_f64": B * M * 8, "sym_f32": B * M * 4},
           "host_chunks_last_call": chunks, "bits_equal": bits_equal,
           "host_wall": {k: _stats(v, B) for k, v in host.items()},
           "device_events": {k: _stats(v, B) for k, v in dev.items()}}
    dl, db, dm = (row["device_events"][k] for k in ("d_decode_scl_llr_dev", "d_decode_bicm_dev", "d_demap_kernel_alone"))
    row["demap_share_of_llr_dev"] = dm["median_s"] / dl["median_s"]
    a, b = row["host_wall"]["a_decode_scl_llr_f64_llr"], row["host_wall"]["b_decode_bicm_f64_sym"]
    row["criteria"] = {
        "host_slowest_bicm_faster_than_fastest_llr": b["max_s"] < a["min_s"],
        "dev_trail_s": db["median_s"] - dl["median_s"],
        "dev_allowance_s": (dl["max_s"] - dl["min_s"]) + dm["median_s"],
        "dev_trail_within_allowance": (db["median_s"] - dl["median_s"]) <= (dl["max_s"] - dl["min_s"]) + dm["median_s"],
    }
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bicm_rx", "rates.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    if a.reps < 5 and not a.quick:
        raise SystemExit("at least 5 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("tools/bicm_rx_rates.py measures on a GPU; none is visible")
    torch.cuda.set_device(0)
    import ctypes
    import golden_util as G
    _, frozen, order, _ = G.tables("cfg5_n10_k512_ask16")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", polar_amd.PolarWeakLeavesWarning)
        cfg5 = polar_amd.PolarCode.from_tables(10, 512, 0, frozen, order, None)
    ctypes.CDLL(None).srand(ctypes.c_uint(1))
    head = polar_amd.PolarCode(11, 1024, 0.32, 16)
    Bs = (8192,) if a.quick else (65536, 262144)
    rows = []
    for name, g, const, snr, L in (("cfg5", cfg5, "ask16-gray", 12.5, 1), ("cfg5", cfg5, "ask16-gray", 12.5, 8),
                                   ("headline_n2048", head, "ask4-gray", 5.0, 32)):
        for B in Bs:
            rows.append(measure(name, g, const, snr, L, B, a.reps))
            r = rows[-1]
            print(json.dumps({"workload": name, "L": L, "B": B, "bits_equal": r["bits_equal"],
                              **{k: round(v["median_cw_per_s"]) for k, v in {**r["host_wall"], **r["device_events"]}.items()},
                              "criteria": r["criteria"]}), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
