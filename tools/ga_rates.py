#!/usr/bin/env python3
"""tools/ga_rates.py — PolarM's main_GA_CC_Comparison.m grid (N = 1024, 7 rates, SNR -10 : 0.25 : 30 dB, target BLER 1e-5,
phi step 1e-5, ask4-gray/bicm, ask4-sp/mlc, ask16-gray/bicm, ask16-sp/mlc) through polar_amd.ga_rate_table on the GPU,
timed end to end (capacities, phi tables, 644 constructions, walks), and the same driver through the numpy restatement
(tests/ga_numpy.py) on one host core, fed the reference's cached polarized capacities (tests/golden/ga_capacity.npz) as
the reference driver is. Writes profiles/ga/ga_rates.json. Per-kernel times: run this under
`rocprofv3 --kernel-trace --stats -- python tools/ga_rates.py --device-only`."""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402


def main():
    out = {}
    import polar_amd
    polar_amd.ga_rate_table()                                  # warm-up (library load, BPSK table of the process)
    walls = []
    for _ in range(3):
        t = time.perf_counter()
        res = polar_amd.ga_rate_table()
        walls.append(time.perf_counter() - t)
    out["device_wall_s"] = walls
    out["device_snr_needed"] = res["snr_needed"].tolist()
    # one design point at the largest supported N (the rank sort is O(N^2) per point, one block per point) and at N = 1024,
    # capacities given: construction only (phi tables included)
    for n in (10, 15):
        polar_amd.ga_construction(n, [5.0], "bpsk", capacity=[[0.8]])
        t = time.perf_counter()
        polar_amd.ga_construction(n, [5.0], "bpsk", capacity=[[0.8]])
        out[f"device_one_point_n{n}_wall_s"] = time.perf_counter() - t
    out["device_ebno_needed"] = res["ebno_needed"].tolist()
    if "--device-only" not in sys.argv:
        import ga_numpy as G
        import mlc_numpy as R
        fix = np.load(os.path.join(ROOT, "tests", "golden", "ga_capacity.npz"))
        rates = [1 / 32, 1 / 16, 1 / 8, 1 / 4, 2 / 4, 3 / 4, 7 / 8]
        snr = -10.0 + np.arange(161) * 0.25
        t = time.perf_counter()
        fwd, inv = G.phi_fwd(), G.phi_inv(1e-5)
        tab = np.array([G.bpsk_cap(s) for s in G.BPSK_SNR])
        host = []
        for name, rx in (("ask4-gray", "bicm"), ("ask4-sp", "mlc"), ("ask16-gray", "bicm"), ("ask16-sp", "mlc")):
            cid = R.NAMES[name]
            nb = R.nbits(cid)
            bler = np.full((161, 7), np.nan)
            for i, s in enumerate(snr):
                if rx == "mlc":
                    cap = G.mlc_capacity(cid, s)
                else:
                    m = (fix["pol_const"] == name) & (fix["pol_snr"] == s)
                    if not m.any():
                        continue
                    cap = fix["pol_cap"][m][0][:nb]
                _, _, pre = G.ga_design(1024, nb, cap, tab, fwd, inv)
                bler[i] = pre[[math.ceil(r * 1024) - 1 for r in rates]]
            host.append(G.rate_walk(bler, rates, snr, 1e-5, nb)[0].tolist())
        out["numpy_one_core_wall_s"] = time.perf_counter() - t
        out["numpy_note"] = ("restatement, one host core, polarized capacities from the reference's cache (not recomputed), "
                             "BPSK table and phi tables computed")
        # what recomputing them would add: one 250 000-symbol point through the restatement, times the 322 points
        t = time.perf_counter()
        G.polarized_counts(R.NAMES["ask16-gray"], 10.0, 1, 0, 250000)
        one = time.perf_counter() - t
        out["numpy_polarized_one_point_s"] = one
        out["numpy_polarized_322_points_estimate_s"] = one * 322
        out["numpy_snr_needed"] = host
    os.makedirs(os.path.join(ROOT, "profiles", "ga"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ga", "ga_rates.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if "wall" in k}))


if __name__ == "__main__":
    main()
