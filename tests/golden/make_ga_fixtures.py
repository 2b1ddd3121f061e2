#!/usr/bin/env python3
"""tests/golden/make_ga_fixtures.py — the caches the reference's Gaussian-approximation construction reads, as one small data
fixture, tests/golden/ga_capacity.npz:
  bpsk_cap       [4001][2]  CapacityHelper/bpsk_cap.mat (snr_vec_db, capacity), the table of get_bpsk_llr_for_capacity.m;
  pol_const      [220]      constellation of each PolarizedCapacityData/<const>_snr_<snr>.mat file,
  pol_snr        [220]      its SNR (dB),
  pol_cap        [220][4]   its cap_vec (get_polarized_capacity, 250 000 symbols; NaN-padded for 4-ASK).
Data only; run HERE with scipy (the reference tree does not travel to the GPU box)."""
import glob
import os
import re

import numpy as np
import scipy.io

SRC = "/root/reference/PolarM/CapacityHelper"
HERE = os.path.dirname(os.path.abspath(__file__))
d = scipy.io.loadmat(os.path.join(SRC, "bpsk_cap.mat"))
bpsk = np.stack([d["snr_vec_db"].reshape(-1), d["capacity"].reshape(-1)], axis=1).astype(np.float64)
assert bpsk.shape == (4001, 2)
rows = []
for f in glob.glob(os.path.join(SRC, "PolarizedCapacityData", "*.mat")):
    m = re.match(r"([a-z0-9-]+)_snr_(-?[\d.]+)\.mat$", os.path.basename(f))
    cap = scipy.io.loadmat(f)["cap_vec"].reshape(-1).astype(np.float64)
    rows.append((m.group(1), float(m.group(2)), np.pad(cap, (0, 4 - cap.size), constant_values=np.nan)))
rows.sort(key=lambda r: (r[0], r[1]))
np.savez_compressed(os.path.join(HERE, "ga_capacity.npz"), bpsk_cap=bpsk, pol_const=np.array([r[0] for r in rows]),
                    pol_snr=np.array([r[1] for r in rows]), pol_cap=np.stack([r[2] for r in rows]))
print(len(rows), "polarized capacities;", sorted(set(r[0] for r in rows)))
