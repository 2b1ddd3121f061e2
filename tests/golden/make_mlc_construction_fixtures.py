#!/usr/bin/env python3
"""tests/golden/make_mlc_construction_fixtures.py — the Monte-Carlo construction tables the reference SHIPS for the
multi-level-coding receiver (PolarM/CodeConstructionData/MC_block_length_1024_512_*_mlc*.txt: per-position error counts of the
genie-aided multistage SC decoder, layer-major, written by PolarCode.m:120-124 from PolarCode.m:155-161, 180-190) as one small
data fixture, tests/golden/construction_tables_mlc.npz. Data only (integers); run HERE (the reference tree does not travel to
the GPU box). Same layout and run-count rule as make_construction_fixtures.py (no `_<runs>` in the name: the default 100e3)."""
import glob
import os
import re

import numpy as np

SRC = "/root/reference/PolarM/CodeConstructionData"
HERE = os.path.dirname(os.path.abspath(__file__))
out = {}
names = []
for f in sorted(glob.glob(os.path.join(SRC, "MC_block_length_1024_512_*_mlc*.txt"))):
    m = re.match(r"MC_block_length_1024_512_cc_method_monte-carlo_cc_param_(-?[\d.]+)_([a-z0-9-]+)_mlc(?:_(\d+))?\.txt", os.path.basename(f))
    snr, const, runs = float(m.group(1)), m.group(2), int(m.group(3) or 100000)
    key = f"{const}_{m.group(1)}_{runs}"
    counts = np.loadtxt(f).astype(np.int64)
    assert counts.size == 1024
    out[key + "/counts"] = counts.astype(np.int32)
    out[key + "/meta"] = np.array([snr, runs], np.float64)
    names.append((key, os.path.basename(f)))
out["keys"] = np.array([k for k, _ in names])
out["files"] = np.array([f for _, f in names])
np.savez_compressed(os.path.join(HERE, "construction_tables_mlc.npz"), **out)
print(len(names), "tables:", [k for k, _ in names])
