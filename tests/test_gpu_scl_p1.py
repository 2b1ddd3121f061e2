"""GPU suite: decode_scl_p1 (scl_decode_p1_kernel<GS>, polar_kernels_p1.hip) against the oracle, bit for bit, at the shapes and
rows its branches special-case: N < 128 (all partial sums in one register), n >= 12 (the deep walk over the HBM partial sums),
list sizes that are no power of two (idle lanes inside a group), sigma == 0 (no normalisation, path 0 wins), ties (the exact
fast path must hand over to the ranking loop), and the second trip of the grid-stride loop (per-wave scratch reused without
clearing). tests/test_p1_oracle.py shows the oracle to be the unmodified reference on every row family used here.
Every batch comes from p1_rows.rows: ordinary rows with the six degenerate rows written over the first ones; ordinary rows,
degenerate rows and their neighbours are all asserted equal to the oracle."""
import numpy as np
import pytest

import p1_rows

pytestmark = pytest.mark.gpu


def _check(o, g, p1, p0, L, what):
    got = g.decode_scl_p1(p1, p0, L)
    assert got.shape == (p1.shape[0], o.K)
    want = np.stack([o.decode_scl_p1(p1[i], p0[i], L) for i in range(p1.shape[0])])
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size}/{p1.shape[0]} rows differ from the oracle (first {bad[:8]}) L={L} {what}"
    return got


@pytest.mark.parametrize("n,K,crc", [(1, 1, 0), (2, 2, 0), (2, 3, 0), (3, 4, 0), (3, 5, 1), (3, 8, 0), (4, 11, 2), (4, 1, 0)])
def test_tiny_block_lengths(built_lib, oracle_built, n, K, crc):
    """N < 128: no HBM partial sums at all; list sizes larger than 2^K never fill, so lanes (path 0 among them) stay idle to the end."""
    o, g = p1_rows.pair(n, K, crc)
    p1, p0 = p1_rows.rows(o, 24, 1.0)
    for L in (1, 2, 3, 4, 8, 32, 64):
        _check(o, g, p1, p0, L, (n, K, crc))


@pytest.mark.parametrize("n,K,crc", [(7, 64, 8), (9, 256, 8)])
@pytest.mark.parametrize("L", [3, 5, 6, 7, 12, 20, 33, 64])
def test_odd_list_sizes(built_lib, oracle_built, n, K, crc, L):
    """Groups wider than the list (rho, need, idle lanes). At -1 dB few visits pass the fast path's strict test; at 4 dB most do."""
    o, g = p1_rows.pair(n, K, crc)
    for ebno in (-1.0, 1.0, 4.0):
        p1, p0 = p1_rows.rows(o, 40, ebno)
        _check(o, g, p1, p0, L, (n, K, crc, ebno))


@pytest.mark.parametrize("L", [4, 32, 64])
def test_ragged_batches_and_empty(built_lib, oracle_built, L):
    """16, 2 and 1 codewords per wave: last waves with idle groups, a batch of one, an empty batch."""
    o, g = p1_rows.pair(6, 30, 4)
    p1, p0 = p1_rows.rows(o, 131, 1.0)
    for B in (1, 2, 3, 7, 9, 63, 65, 131):
        _check(o, g, p1[:B], p0[:B], L, B)
    assert g.decode_scl_p1(p1[:0], p0[:0], L).shape == (0, 30)


@pytest.mark.parametrize("L", [64, 32])
def test_more_codewords_than_waves(built_lib, oracle_built, L):
    """Every wave decodes a second and a third codeword: the path history, the layers and the free-slot stack of the codeword
    before are still in its scratch. A degenerate row every 97 rows, so that what it leaves behind meets an ordinary row (and the reverse)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    o, g = p1_rows.pair(5, 16, 4)
    gs = 64 if L == 64 else 32
    B = 2 * 16 * cus * (64 // gs) + 5
    p1, p0 = p1_rows.rows(o, B, 1.0, every=97)
    _check(o, g, p1, p0, L, B)


@pytest.mark.parametrize("n,K,crc,L,B", [(12, 2048, 16, 4, 6), (12, 2048, 16, 32, 6), (13, 4096, 0, 2, 4)])
def test_long_codes(built_lib, oracle_built, n, K, crc, L, B):
    """n >= 12: the partial-sum walk over the HBM words runs deeper than any n = 11 code takes it."""
    o, g = p1_rows.pair(n, K, crc)
    for ebno in (2.0, -1.0):
        p1, p0 = p1_rows.rows(o, B, ebno)
        _check(o, g, p1, p0, L, (n, K, crc, ebno))


def test_agrees_with_the_llr_decoder_as_often_as_the_oracle_does(built_lib, oracle_built):
    """Ordinary rows: the probability-domain decoder is another arithmetic than the LLR one, so agreement is on decisions and need
    not be total. Bar: the device differs from decode_scl_llr on no more rows than the oracle's own decode_scl_p1 does on the same
    inputs (and it equals the oracle row for row, so the counts are the same; the printed number is informational)."""
    o, g = p1_rows.pair(10, 512, 8)
    llr, _ = o.synth_llr(2222, 0, 256, o.snr_sqrt_linear(2.5))
    p1 = 1.0 / (1.0 + np.exp(llr))
    p0 = 1.0 - p1
    by_llr = g.decode_scl_llr(llr, 8)
    got = g.decode_scl_p1(p1, p0, 8)
    want = np.stack([o.decode_scl_p1(p1[i], p0[i], 8) for i in range(256)])
    dev = int((got != by_llr).any(axis=1).sum())
    orc = int((want != by_llr).any(axis=1).sum())
    print(f"rows of 256 where decode_scl_p1 differs from decode_scl_llr: device {dev}, oracle {orc}")
    assert dev <= orc
    assert (got == want).all()
