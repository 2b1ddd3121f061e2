"""GPU: the front of the Monte-Carlo path (polar_amd/csrc/polar_channel.hip: encode_kernel, synth_kernel on its BPSK and ASK
paths, count_errors_kernel) at the shapes where its lane loops, its LDS image and its grid-stride loops can go wrong: N and K below
the 64 lanes, K next to 64 and 128 (the 128-bit info words of polar_synth_info_word), CRCs as wide as a short K allows, batches of
more than 8192 rows (later trips of a block reuse the LDS image), trial indices beyond 2^32 with the every-100-trials info
refresh, and the label tail of 8-ASK. Every comparison is bit for bit, doubles as 64-bit patterns, with the numpy models of
tests/sweep_numpy.py and the oracle. All of sweep_numpy.FRONT_CODES are accepted by the handle: none is dropped."""
import functools

import numpy as np
import pytest

import sweep_numpy as S

pytestmark = pytest.mark.gpu

GRID = 8192                                   # blocks of a launch at the most (grid_for, polar_channel.hip)
TRIALS = (0, 95, 2**32 - 3, 2**40 + 99)       # B = 10 from these: across an info refresh (95, 2^40 + 99: trial / 100 steps) or across 2^32
code_id = lambda c: "n%d_k%d_crc%d" % c


@functools.lru_cache(maxsize=None)
def _pair(code):
    import p1_rows
    return p1_rows.pair(*code)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(B, width, dtype, fill):
    """a device tensor of B + 1 rows filled with a sentinel: the kernel under test writes exactly B of them"""
    import torch
    return torch.full((B + 1, width), fill, dtype=dtype, device="cuda")


LLR_GUARD, INFO_GUARD = -7.25, 0xA5


@pytest.mark.parametrize("code", S.FRONT_CODES, ids=code_id)
def test_encoder_equals_the_numpy_model(built_lib, oracle_built, code):
    """encode (host rows) and encode_dev (device rows) at B = 1 and 37, and at 2 * 8192 + 3 rows — a second and a third trip of the
    blocks — for N = 32 and for K = 65"""
    import torch
    n, K, crc = code
    o, g = _pair(code)
    order, crcm = o.order(), o.crc_matrix()
    sizes = (1, 37) + ((2 * GRID + 3,) if code in ((5, 16, 0), (7, 65, 0)) else ())
    for B in sizes:
        info = S.info_rows(K, B, 5 * B + K)
        want = S.encode(order, crcm, n, info)
        assert np.array_equal(g.encode(info), want), B
        d_info, d_coded = _dev(info), _guarded(B, g.N, torch.uint8, INFO_GUARD)
        g.encode_dev(d_info.data_ptr(), B, d_coded.data_ptr())
        torch.cuda.synchronize()
        got = d_coded.cpu().numpy()
        bad = np.nonzero((got[:B] != want).any(axis=1))[0]
        assert bad.size == 0, (B, bad[:8])
        assert (got[B] == INFO_GUARD).all()
    # no rows: nothing is launched, nothing is written
    d_info, d_coded = _dev(np.zeros((1, K), np.uint8)), _guarded(1, g.N, torch.uint8, INFO_GUARD)
    g.encode_dev(d_info.data_ptr(), 0, d_coded.data_ptr())
    torch.cuda.synchronize()
    assert (d_coded.cpu().numpy() == INFO_GUARD).all()


def _synth_check(o, g, seed, t0, B, ebno, with_info=True):
    import torch
    s = o.snr_sqrt_linear(ebno)
    assert s == g.snr_sqrt_linear(ebno)
    llr, info = o.synth_llr(seed, t0, B, s)
    d_llr = _guarded(B, g.N, torch.float64, LLR_GUARD)
    d_info = _guarded(B, g.K, torch.uint8, INFO_GUARD)
    g.synth_llr_dev(seed, t0, B, s, d_llr.data_ptr(), d_info.data_ptr() if with_info else 0)
    torch.cuda.synchronize()
    got, got_info = d_llr.cpu().numpy(), d_info.cpu().numpy()
    bad = np.nonzero((_bits(got[:B]) != _bits(llr)).any(axis=1))[0]
    assert bad.size == 0, (t0, ebno, B, bad[:8])
    assert (_bits(got[B]) == _bits(np.float64(LLR_GUARD))).all(), (t0, ebno, B)
    if with_info:
        bad = np.nonzero((got_info[:B] != info).any(axis=1))[0]
        assert bad.size == 0, (t0, ebno, B, bad[:8])
        assert (got_info[B] == INFO_GUARD).all()
    else:
        assert (got_info == INFO_GUARD).all()
    return info


@pytest.mark.parametrize("code", S.FRONT_CODES, ids=code_id)
def test_bpsk_synth_equals_the_oracle(built_lib, oracle_built, code):
    """synth_llr_dev: LLR and info rows of 10 trials from each of TRIALS at two Eb/N0, the row behind the last one untouched; once
    without the info output; at N = 32 also 8192 + 70 rows, compared in full (the blocks' second trip)"""
    o, g = _pair(code)
    for t0 in TRIALS:
        for ebno in (0.0, 2.5):
            info = _synth_check(o, g, 4242, t0, 10, ebno)
        if t0 == 95 and g.K >= 16:          # (the refresh is in the inputs: trials 99 and 100 carry different info)
            assert (info[0] == info[4]).all() and (info[4] != info[5]).any() and (info[5] == info[9]).all()
    _synth_check(o, g, 4242, 2**32 - 3, 10, 2.5, with_info=False)
    if code == (5, 16, 0):
        _synth_check(o, g, 77, 2**32 - 5000, GRID + 70, 0.0)


NBITS = {1: 2, 2: 3, 3: 4}


@pytest.mark.parametrize("cid", [1, 2, 3])
@pytest.mark.parametrize("code", S.ASK_CODES, ids=code_id)
def test_ask_synth_equals_the_oracle_and_its_symbols_demap_to_its_llrs(built_lib, oracle_built, code, cid):
    """synth_bicm_llr_dev against the oracle with few symbols (1, 21, 42) and more than 64 (85), the N mod n_bits tail positions
    exactly +0.0; synth_bicm_sym_dev the way tests/test_gpu_bicm_rx.py checks it: its symbols, demapped on the device, are the
    LLR rows bit for bit"""
    import torch
    import polar_amd
    o, g = _pair(code)
    con = polar_amd.Constellation(cid)
    N, B, nb = g.N, 10, NBITS[cid]
    M = N // nb
    assert M >= 1
    for t0 in (0, 2**32 - 3):
        for snr in (6.0, 11.5):
            llr, info = o.synth_bicm_llr(cid, 31, t0, B, snr)
            d_llr = _guarded(B, N, torch.float64, LLR_GUARD)
            d_info = _guarded(B, g.K, torch.uint8, INFO_GUARD)
            g.synth_bicm_llr_dev(cid, 31, t0, B, snr, d_llr.data_ptr(), d_info.data_ptr())
            d_y = _guarded(B, M, torch.float64, LLR_GUARD)
            d_info2 = _guarded(B, g.K, torch.uint8, INFO_GUARD)
            g.synth_bicm_sym_dev(cid, 31, t0, B, snr, d_y.data_ptr(), d_info2.data_ptr())
            torch.cuda.synchronize()
            got, got_info = d_llr.cpu().numpy(), d_info.cpu().numpy()
            assert (_bits(got[:B]) == _bits(llr)).all(), (t0, snr)
            assert (_bits(got[:B, M * nb:]) == 0).all()                 # (+0.0, not -0.0)
            assert (_bits(got[B]) == _bits(np.float64(LLR_GUARD))).all()
            assert (got_info[:B] == info).all() and (got_info[B] == INFO_GUARD).all()
            assert torch.equal(d_info2, d_info)
            y = d_y.cpu().numpy()
            assert np.isfinite(y[:B]).all() and (_bits(y[B]) == _bits(np.float64(LLR_GUARD))).all()
            sigma = np.sqrt(0.5) * 10 ** (-snr / 20)                   # main_MC_CC_Comparison.m:90
            again = torch.full((B, N), LLR_GUARD, dtype=torch.float64, device="cuda")
            con.compute_llr_bicm_dev(d_y.data_ptr(), N, B, sigma * sigma, again.data_ptr())
            torch.cuda.synchronize()
            assert (_bits(again.cpu().numpy()) == _bits(llr)).all(), (t0, snr)


@pytest.mark.parametrize("cid", [2, 3])
def test_ask_rows_shorter_than_one_label_are_all_tail(built_lib, oracle_built, cid):
    """N = 2 under 3- and 4-bit labels: no symbol fits. The library accepts the call; the rows are the tail's +0.0 throughout (as
    the oracle's), the info rows are generated all the same."""
    import torch
    o, g = _pair((1, 1, 0))
    llr, info = o.synth_bicm_llr(cid, 31, 2**32 - 3, 10, 6.0)
    assert (_bits(llr) == 0).all()
    d_llr = _guarded(10, 2, torch.float64, LLR_GUARD)
    d_info = _guarded(10, 1, torch.uint8, INFO_GUARD)
    g.synth_bicm_llr_dev(cid, 31, 2**32 - 3, 10, 6.0, d_llr.data_ptr(), d_info.data_ptr())
    torch.cuda.synchronize()
    got = d_llr.cpu().numpy()
    assert (_bits(got[:10]) == 0).all() and (_bits(got[10]) == _bits(np.float64(LLR_GUARD))).all()
    assert (d_info.cpu().numpy()[:10] == info).all() and int(d_info[10, 0]) == INFO_GUARD


def _error_rows(K, B, seed):
    """(a, b): decoded and sent rows of K bytes. Row r < 6 (as B holds them) is of kind r: identical; byte 0 differs; byte K - 1;
    byte 64 (K > 64, else K // 2); every byte; byte K - 1 is 2 against 0. Of the rest about a third differ, in one random byte."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2, (B, K)).astype(np.uint8)
    b = a.copy()
    pick = rng.random(B) < 1 / 3
    pos = rng.integers(0, K, B)
    rows = np.nonzero(pick)[0]
    b[rows, pos[rows]] ^= 1
    for r in range(min(B, 6)):
        b[r] = a[r]
        if r == 1:
            b[r, 0] ^= 1
        elif r == 2:
            b[r, K - 1] ^= 1
        elif r == 3:
            b[r, 64 if K > 64 else K // 2] ^= 1
        elif r == 4:
            b[r] ^= 1
        elif r == 5:
            a[r, K - 1], b[r, K - 1] = 2, 0
    return a, b


@pytest.mark.parametrize("code", [(1, 2, 0), (6, 1, 0), (7, 63, 0), (7, 64, 8), (7, 65, 0), (8, 129, 3), (8, 200, 16)], ids=code_id)
def test_error_count_equals_the_numpy_model_and_accumulates(built_lib, oracle_built, code):
    """count_errors_dev: rows that differ in the first, the last, the 65th, every byte, by value and not by bit; 1, 5 and 8192 + 5
    rows; the counter is added to — from zero, from a value, twice in a row — and left alone by an empty batch"""
    import torch
    K = code[1]
    o, g = _pair(code)
    for B, start in ((1, 0), (5, 0), (5, 10**12 + 7), (GRID + 5, 3)):
        a, b = _error_rows(K, B, 13 * B + K)
        flags, want = S.count_errors(a, b)
        if B >= 5:
            assert flags[:5].tolist() == [False, True, True, True, True] and (B < 6 or flags[5])
        d_a, d_b = _dev(a), _dev(b)
        ctr = torch.tensor([start, 99], dtype=torch.int64, device="cuda")
        g.count_errors_dev(d_a.data_ptr(), d_b.data_ptr(), B, ctr.data_ptr())
        torch.cuda.synchronize()
        assert ctr.tolist() == [start + want, 99], (B, start)
        g.count_errors_dev(d_b.data_ptr(), d_a.data_ptr(), B, ctr.data_ptr())            # (the kernel accumulates: bench.py's steps)
        g.count_errors_dev(d_a.data_ptr(), d_a.data_ptr(), B, ctr.data_ptr())
        g.count_errors_dev(d_a.data_ptr(), d_b.data_ptr(), 0, ctr.data_ptr())
        torch.cuda.synchronize()
        assert ctr.tolist() == [start + 2 * want, 99], (B, start)
        if B > 1:        # one row further on: each row is compared with the wrong one, and the model says what that gives
            shifted = np.roll(b, 1, axis=0)
            d_s = _dev(shifted)
            ctr.zero_()
            g.count_errors_dev(d_a.data_ptr(), d_s.data_ptr(), B, ctr.data_ptr())
            torch.cuda.synchronize()
            assert ctr.tolist() == [S.count_errors(a, shifted)[1], 0]
