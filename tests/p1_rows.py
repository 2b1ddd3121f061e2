"""Input rows shared by the probability-domain tests (test_p1_oracle.py, test_gpu_scl_p1.py, test_gpu_sc_p1.py): ordinary rows
p1 = 1 / (1 + e^llr), p0 = 1 - p1 from the oracle's synthetic channel, and the degenerate rows the kernels of
polar_kernels_p1.hip special-case. Every comparison built on them is equality of bits or of doubles."""
import ctypes as C

import numpy as np

EDGE_KINDS = ("half", "zero_one", "extremes", "zeros", "quarters", "scaled")


def oracle(n, K, crc, srand=1):
    from oracle_lib import Oracle
    return Oracle(n, K, 0.32, crc, srand=srand)


def pair(n, K, crc, srand=1):
    """(oracle, device code) with the same construction."""
    import polar_amd
    o = oracle(n, K, crc, srand)
    C.CDLL(None).srand(C.c_uint(srand))
    return o, polar_amd.PolarCode(n, K, 0.32, crc)


def edge_row(kind, p1_row):
    """The degenerate row `kind`, made from (and as long as) the ordinary row p1_row: (p1, p0)."""
    N = p1_row.shape[0]
    i = np.arange(N)
    if kind == "half":                  # every fork of every path ties
        p1 = np.full(N, 0.5)
        return p1, p1.copy()
    if kind == "zero_one":              # certain inputs: exact-zero products in SCL (sigma reaches 0); 0 / 0 in vnop for SC, already at n = 1
        p1 = (i & 1).astype(np.float64)
        return p1, 1.0 - p1
    if kind == "extremes":              # 1e-300 / 1 - 1e-16 in a period of three
        p1 = np.where(i % 3 == 0, 1e-300, 1.0 - 1e-16)
        return p1, 1.0 - p1
    if kind == "zeros":                 # p0 = p1 = 0: sigma == 0 in every layer, nothing is normalised, no path beats 0 at the end
        return np.zeros(N), np.zeros(N)
    if kind == "quarters":              # p1 rounded to quarters: equal forks within and across paths
        p1 = np.round(p1_row * 4.0) / 4.0
        return p1, 1.0 - p1
    if kind == "scaled":                # both scaled by 1e-150: only the normalisation keeps the products from underflowing
        return p1_row * 1e-150, (1.0 - p1_row) * 1e-150
    raise ValueError(kind)


def rows(o, B, ebno, seed=2222, every=0):
    """B rows (p1, p0) at Eb/N0 = ebno dB. The degenerate rows overwrite the first ones (as many as B holds); with every > 0
    they also overwrite rows every, 2 * every, ... in turn, so that each has ordinary neighbours decoded before and after it
    by the same wave."""
    llr, _ = o.synth_llr(seed, 0, B, o.snr_sqrt_linear(ebno))
    with np.errstate(over="ignore"):
        p1 = 1.0 / (1.0 + np.exp(llr))
    p0 = 1.0 - p1
    where = [(k, k) for k in range(min(B, len(EDGE_KINDS)))]
    if every:
        where += [(r, (r // every - 1) % len(EDGE_KINDS)) for r in range(every, B, every)]
    for r, k in where:
        p1[r], p0[r] = edge_row(EDGE_KINDS[k], p1[r].copy())
    return p1, p0


def rows_that_differ(got, want):
    """Rows (indices) where two arrays of doubles differ: NaN positions are compared apart from the values, so that a NaN's sign
    or payload cannot matter."""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (got != want))
    return np.nonzero(bad.any(axis=1))[0]
