"""SC-Flip on the device (polar_decode_sc_flip_batch[_dev], polar_mc_batch_flip) against the numpy model of tests/flip_numpy.py, the
library's own list call at L = 1 and decode_scl_llr itself."""
import os
import subprocess

import numpy as np
import pytest

import flip_numpy as F
import scl_list_numpy as S

pytestmark = pytest.mark.gpu
REL = 1e-10          # libm against the kernel's table-driven exp / log1p: the tolerance of test_gpu_scl_list.py
SENT = 0xA5          # sentinel byte of the output buffers


def _pair(n, K, crc, srand=1):
    import ctypes as C
    import polar_amd
    from oracle_lib import Oracle
    o = Oracle(n, K, 0.32, crc, srand=srand)
    C.CDLL(None).srand(C.c_uint(srand))
    g = polar_amd.PolarCode(n, K, 0.32, crc)
    return o, g


def _same_as_model(got, r, rows=None):
    """words, crc_ok, n_dec, flip and cand exactly, mag to REL; `got` = (out, crc_ok, n_dec, flip, cand, mag) of len(r) rows."""
    out, ok, nd, flip, cand, mag = got
    assert (out == r["info"]).all() and (ok == r["crc_ok"]).all() and (nd == r["n_dec"]).all() and (flip == r["flip"]).all()
    assert (cand == r["cand"]).all()
    fin = np.isfinite(r["mag"])
    assert (np.isposinf(mag) == ~fin).all()
    assert (np.abs(mag[fin] - r["mag"][fin]) <= REL * np.maximum(1.0, np.abs(r["mag"][fin]))).all()


def _buffers(B, K, T):
    import torch
    return (torch.full((B + 1, K), SENT, dtype=torch.uint8, device="cuda"), torch.full((B + 1,), SENT, dtype=torch.uint8, device="cuda"),
            torch.full((B + 1,), SENT, dtype=torch.uint8, device="cuda"), torch.full((B + 1,), -7, dtype=torch.int32, device="cuda"),
            torch.full((B + 1, T), -7, dtype=torch.int32, device="cuda"), torch.full((B + 1, T), -1.0, dtype=torch.float64, device="cuda"))


def _launch(g, t, fmt, B, T, bufs, use=(True,) * 5, stream=None):
    g.decode_sc_flip_dev(t.data_ptr(), fmt, B, T, bufs[0].data_ptr(), *[b.data_ptr() if u else 0 for b, u in zip(bufs[1:], use)],
                         stream=stream)


def _fetch(bufs, use=(True,) * 5):
    return [bufs[0].cpu().numpy()] + [b.cpu().numpy() if u else None for b, u in zip(bufs[1:], use)]


def _dev(g, t, fmt, B, T, use=(True,) * 5, stream=None):
    """The _dev call into sentinel-filled buffers with one row of slack: (out, crc_ok, n_dec, flip, cand, mag) of B + 1 rows (None for
    an output left out), after a synchronisation."""
    import torch
    bufs = _buffers(B, g.K, T)
    _launch(g, t, fmt, B, T, bufs, use, stream)
    torch.cuda.synchronize()
    return _fetch(bufs, use)


def _check_slack(got, B, T, te):
    """Every row below B is written, the slack row is untouched."""
    out, ok, nd, flip, cand, mag = got
    assert (out[:B] <= 1).all() and (out[B] == SENT).all()
    if ok is not None:
        assert (ok[:B] <= 1).all() and ok[B] == SENT
    if nd is not None:
        assert (nd[:B] >= 1).all() and (nd[:B] <= te + 1).all() and nd[B] == SENT
    if flip is not None:
        assert (flip[:B] >= -1).all() and flip[B] == -7
    if cand is not None:
        assert (cand[:B, :te] >= 0).all() and (cand[:B, te:] == -1).all() and (cand[B] == -7).all()
    if mag is not None:
        assert (mag[:B, :te] >= 0).all() and np.isposinf(mag[:B, te:]).all() and (mag[B] == -1.0).all()


def _synth(g, seed, B, ebno, N, info=False):
    import torch
    t = torch.empty((B, N), dtype=torch.float64, device="cuda")
    sent = torch.empty((B, g.K), dtype=torch.uint8, device="cuda") if info else None
    g.synth_llr_dev(seed, 0, B, g.snr_sqrt_linear(ebno), t.data_ptr(), sent.data_ptr() if info else 0)
    torch.cuda.synchronize()
    return (t, sent.cpu().numpy()) if info else t


# ---- 1. against numpy: the table rows and the stored fixtures ----------------------------------------------------------------------
@pytest.mark.parametrize("key,T,share,err,undet,dec", F.TABLE)
def test_table_rows_equal_numpy(built_lib, oracle_built, key, T, share, err, undet, dec):
    o, code, llr, sent, r = F.reference(key, T)
    _, g = _pair(*key)
    got = g.decode_sc_flip(llr, T, return_candidates=True)
    print(key, T, "device n_dec", np.bincount(got[2], minlength=T + 2).tolist(), "numpy", F.TABLE_HIST[(key, T)])
    _same_as_model(got, r)
    assert np.bincount(got[2], minlength=T + 2).tolist() == F.TABLE_HIST[(key, T)]
    res = dict(info=got[0], crc_ok=got[1], n_dec=got[2])
    assert F.shares(res) == share and F.counters(res, sent).tolist() == [256, err, undet, share[0], share[1], dec]


@pytest.mark.parametrize("i", range(len(F.FIXTURES)))
def test_fixture_rows_equal_numpy(built_lib, oracle_built, i):
    rows, key, T, seed, ebno, share = F.FIXTURES[i]
    o, g = _pair(*key)
    llr, sent = o.synth_llr(seed, 0, rows, o.snr_sqrt_linear(ebno))
    fx = F.load_fixtures()[i]
    assert (fx["llr_sha"] == F.llr_sha(llr)).all() and (fx["sent"] == sent).all() and len(fx["info"]) == rows
    got = g.decode_sc_flip(llr, T, return_candidates=True)
    print(key, T, ebno, "device", F.shares(dict(info=got[0], crc_ok=got[1], n_dec=got[2])), "stored", share)
    _same_as_model(got, fx)
    assert F.shares(dict(info=got[0], crc_ok=got[1], n_dec=got[2])) == share


# ---- 2. against the library's own list-of-1 decode at working shapes ----------------------------------------------------------------
@pytest.fixture(scope="module")
def working(built_lib, oracle_built):
    """Per code: (g, rows on the device, the list call at L = 1, the T = 0 call, the T = 8 call), computed once."""
    import torch
    res = {}
    for key in ((10, 512, 8), (11, 1024, 16)):
        _, g = _pair(*key)
        B, N, K = 256, 1 << key[0], key[1]
        t = _synth(g, 21, B, 1.5, N)
        cand = torch.full((B, 1, K), 7, dtype=torch.uint8, device="cuda")
        ok = torch.full((B, 1), 7, dtype=torch.uint8, device="cuda")
        win = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        g.decode_scl_llr_list_dev(t.data_ptr(), "f64", B, 1, cand.data_ptr(), 0, ok.data_ptr(), 0, win.data_ptr())
        torch.cuda.synchronize()
        res[key] = (g, t, (cand.cpu().numpy()[:, 0], ok.cpu().numpy()[:, 0], win.cpu().numpy()), _dev(g, t, "f64", B, 0), _dev(g, t, "f64", B, 8))
    return res


@pytest.mark.parametrize("key", [(10, 512, 8), (11, 1024, 16)])
def test_no_flips_is_the_list_of_one(working, key):
    g, t, (word, flag, win), r0, r8 = working[key]
    B = 256
    _check_slack(r0, B, 0, 0)
    assert (win == 0).all()
    assert (r0[0][:B] == word).all() and (r0[1][:B] == flag).all() and (r0[2][:B] == 1).all() and (r0[3][:B] == -1).all()
    assert 0 < flag.sum() < B


@pytest.mark.parametrize("key", [(10, 512, 8), (11, 1024, 16)])
def test_flips_against_decode_scl_llr_and_the_call_without(working, key):
    import torch
    g, t, _, r0, r8 = working[key]
    B, K = 256, key[1]
    _check_slack(r8, B, 8, 8)
    out8, ok8, nd8, flip8, cand8, mag8 = (x[:B] for x in r8)
    out = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    g.set_mode(1)
    try:
        g.decode_scl_llr_dev(t.data_ptr(), B, 1, out.data_ptr())
        torch.cuda.synchronize()
    finally:
        g.set_mode(0)
    first, failed = nd8 == 1, ok8 == 0
    print(key, "first", int(first.sum()), "flipped", int(((ok8 == 1) & ~first).sum()), "failed", int(failed.sum()))
    assert first.sum() > 0 and failed.sum() > 0 and ((ok8 == 1) & ~first).sum() > 0
    assert (out.cpu().numpy()[first] == out8[first]).all()
    assert (first == (r0[1][:B] == 1)).all() and (ok8[first] == 1).all()
    assert (out8[failed] == r0[0][:B][failed]).all() and (nd8[failed] == 9).all() and (flip8[failed] == -1).all()
    # a delivered retry flipped the candidate its n_dec names; candidates are unfrozen and their magnitudes ascend
    hit = np.flatnonzero((ok8 == 1) & ~first)
    assert (flip8[hit] == cand8[hit, nd8[hit] - 2]).all()
    assert (g.frozen_bits[cand8] == 0).all() and (np.diff(mag8, axis=1) >= 0).all()


# ---- 3. grid edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", F.EDGE_B)
def test_grid_edges(built_lib, oracle_built, B):
    """(6, 32, 8), T = EDGE_T, the rows of flip_numpy.edge_seed (tests/test_flip.py: the model raises no MarginError on any of them)
    against the model; beside it 8 dB: everything is first-pass, -10 dB: every retry is spent and nothing passes."""
    import torch
    o, g = _pair(6, 32, 8)
    code, T = S.Code(o), F.EDGE_T
    for ebno in F.EDGE_EBNO:
        llr, _ = o.synth_llr(F.edge_seed(B, ebno), 0, B, o.snr_sqrt_linear(ebno))
        got = _dev(g, torch.tensor(llr, device="cuda"), "f64", B, T)
        _check_slack(got, B, T, T)
        out, ok, nd, flip, cand, mag = (x[:B] for x in got)
        print(B, ebno, np.bincount(nd, minlength=T + 2).tolist())
        _same_as_model((out, ok, nd, flip, cand, mag), F.decode(code, llr, T))
        if ebno == 8.0:
            assert (nd == 1).all() and (ok == 1).all() and (flip == -1).all()
        elif ebno == -10.0:
            assert (nd == T + 1).all() and (ok == 0).all() and (flip == -1).all()


def test_above_the_grid_cap(built_lib, oracle_built):
    """One row more than the launch has blocks: the grid-stride loop runs twice in block 0."""
    import torch
    B, seed, ebno, T = F.GRID_CAP_CASE
    o, g = _pair(6, 32, 8)
    llr, sent = o.synth_llr(seed, 0, B, o.snr_sqrt_linear(ebno))
    r = F.decode(S.Code(o), llr, T)
    got = _dev(g, torch.tensor(llr, device="cuda"), "f64", B, T)
    _check_slack(got, B, T, T)
    _same_as_model([x[:B] for x in got], r)
    assert min(F.shares(r)) > 0


# ---- 4. the all-zero row, the min-sum branch, the clamp ---------------------------------------------------------------------------
def test_all_zero_row(built_lib, oracle_built):
    o, g = _pair(5, 16, 8)
    T = 5
    out, ok, nd, flip, cand, mag = g.decode_sc_flip(np.zeros((3, 32)), T, return_candidates=True)
    first = np.flatnonzero(g.frozen_bits == 0)[:T]
    assert (out == 0).all() and (ok == 1).all() and (nd == 1).all() and (flip == -1).all()
    assert (cand == first).all() and (mag == 0).all()


def test_min_sum_branch(built_lib, oracle_built):
    """Rows scaled by 50: every f-node takes the min-sum branch (max(|a|, |b|) >= 40 from the channel on)."""
    key, T = (6, 32, 8), 8
    o, code, llr, sent, _ = F.reference(key, T)
    big = F.MIN_SUM_SCALE * llr[:F.MIN_SUM_ROWS]
    r = F.decode(code, big, T)
    _, g = _pair(*key)
    got = g.decode_sc_flip(big, T, return_candidates=True)
    _same_as_model(got, r)
    assert len(set(r["n_dec"].tolist())) > 1


# ---- 5. optional outputs, two calls on one stream ---------------------------------------------------------------------------------
def test_optional_outputs(built_lib, oracle_built):
    _, g = _pair(6, 32, 8)
    B, T = 65, 8
    t = _synth(g, 41, B, 1.5, 64)
    full = _dev(g, t, "f64", B, T)
    _check_slack(full, B, T, T)
    assert len(set(full[2][:B].tolist())) > 2
    for skip in list(range(5)) + [None]:
        use = tuple(False if skip is None else k != skip for k in range(5))
        got = _dev(g, t, "f64", B, T, use=use)
        _check_slack(got, B, T, T)
        for a, b in zip(got, full):
            assert a is None or a.tobytes() == b.tobytes(), skip


def test_two_calls_on_one_stream(built_lib, oracle_built):
    import torch
    _, g = _pair(6, 32, 8)
    K = 32
    (B1, T1), (B2, T2) = (257, 8), (65, 3)
    t1, t2 = _synth(g, 51, B1, 1.0, 64), _synth(g, 52, B2, 0.5, 64)
    want1, want2 = _dev(g, t1, "f64", B1, T1), _dev(g, t2, "f64", B2, T2)      # (the first call uploads the schedule: nothing allocates below)
    st = torch.cuda.Stream()
    b1, b2 = _buffers(B1, K, T1), _buffers(B2, K, T2)
    torch.cuda.synchronize()
    allocs = g.debug_get("allocs")
    with torch.cuda.stream(st):
        _launch(g, t1, "f64", B1, T1, b1, stream=st)
        _launch(g, t2, "f64", B2, T2, b2, stream=st)
    assert g.debug_get("allocs") == allocs
    torch.cuda.synchronize()
    for got, want in ((_fetch(b1), want1), (_fetch(b2), want2)):
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()
    _check_slack(_fetch(b1), B1, T1, T1)
    _check_slack(_fetch(b2), B2, T2, T2)


# ---- 6. element formats, host form ------------------------------------------------------------------------------------------------
def test_formats_and_host_form(built_lib, oracle_built):
    import torch
    from llr16_util import to_bf16_patterns, widen_bf16
    o, g = _pair(6, 32, 8)
    B, T, K = 65, 8, 32
    llr, _ = o.synth_llr(9, 0, B, o.snr_sqrt_linear(1.5))
    f32 = llr.astype(np.float32)
    f16 = llr.astype(np.float16)
    b16 = to_bf16_patterns(llr)
    for fmt, rows, wide in (("f64", llr, llr), ("f32", f32, f32.astype(np.float64)), ("f16", f16, f16.astype(np.float64)),
                            ("bf16", b16, widen_bf16(b16))):
        want = _dev(g, torch.tensor(wide, device="cuda"), "f64", B, T)
        src = torch.tensor(rows.view(np.int16) if rows.dtype.itemsize == 2 else rows, device="cuda")
        got = _dev(g, src, fmt, B, T)
        _check_slack(got, B, T, T)
        host = g.decode_sc_flip(rows, T, fmt=fmt if fmt == "bf16" else None, return_candidates=True)
        for w, a, h in zip(want, got, host):
            assert w.tobytes() == a.tobytes() and w[:B].tobytes() == h.tobytes(), fmt
        assert len(set(got[2][:B].tolist())) > 1, fmt
    # the host form with outputs left out, called through the C-ABI, and the four-value return
    import ctypes as C
    out = np.zeros((B, K), np.uint8)
    assert g._L.polar_decode_sc_flip_batch(g._h, C.c_void_p(llr.ctypes.data), C.c_int(0), C.c_long(B), C.c_int(T), C.c_void_p(out.ctypes.data),
                                           None, None, None, None, None) == 0
    four = g.decode_sc_flip(llr, T)
    assert len(four) == 4 and (out == four[0]).all()
    six = g.decode_sc_flip(llr, T, return_candidates=True)
    for a, b in zip(four, six):
        assert a.tobytes() == b.tobytes()
    one = g.decode_sc_flip(llr[0], T)
    assert (one[0] == four[0][:1]).all() and one[2][0] == four[2][0]


# ---- 7. sizes -------------------------------------------------------------------------------------------------------------------------
def test_size_limits(built_lib, oracle_built):
    """n = 13 is refused; n = 12 runs (64 KiB of LDS for the layers) and equals the list of 1 at 3 dB; N < 64 runs."""
    import polar_amd
    import torch
    g13 = polar_amd.PolarCode(13, 4096, 0.32, 16)
    with pytest.raises(polar_amd.PolarError, match="-4"):
        g13.decode_sc_flip(np.ones((1, 8192)), 2)
    _, g = _pair(12, 2048, 16)
    B = 8
    t = _synth(g, 3, B, 3.0, 4096)
    got = _dev(g, t, "f64", B, 2)
    _check_slack(got, B, 2, 2)
    word = g.decode_scl_llr_list(t.cpu().numpy(), 1)
    assert (got[0][:B] == word[0][:, 0]).all() and (got[1][:B] == word[2][:, 0]).all() and (got[2][:B] <= 3).all()


# ---- 8. the sweep -----------------------------------------------------------------------------------------------------------------
def _mc(g, T, flips, axis, enabled=None, t0=0, stride=1, constellation=0, seed=1):
    stats = np.zeros((len(axis), 6), np.uint64)
    g.mc_batch_flip(seed, t0, T, stride, axis, flips, np.ones(len(axis), np.uint8) if enabled is None else enabled, stats, constellation)
    return stats


@pytest.mark.parametrize("key,T,share,err,undet,dec", F.TABLE)
def test_sweep_counters_equal_numpy(built_lib, oracle_built, key, T, share, err, undet, dec):
    import list_stats_numpy as LS
    o, code, llr, sent, r = F.reference(key, T)
    want = F.counters(r, sent)
    _, g = _pair(*key)
    n = 256
    got = _mc(g, n, T, [LS.STATS_EBNO], seed=LS.STATS_SEED)[0]
    print(key, T, "device", got.tolist(), "numpy", want.tolist())
    assert got.tolist() == want.tolist() == [256, err, undet, share[0], share[1], dec]
    # chunks of 7 trials
    g.debug_set("list_chunk_cw", 7)
    try:
        assert _mc(g, n, T, [LS.STATS_EBNO], seed=LS.STATS_SEED)[0].tolist() == got.tolist()
    finally:
        g.debug_set("list_chunk_cw", 0)
    # even and odd trials
    halves = _mc(g, n // 2, T, [LS.STATS_EBNO], t0=0, stride=2) + _mc(g, n // 2, T, [LS.STATS_EBNO], t0=1, stride=2)
    assert halves[0].tolist() == got.tolist()


def test_sweep_no_flips_a_disabled_point_and_flip_stats(built_lib, oracle_built):
    _, g = _pair(6, 32, 8)
    n = 256
    ls = np.zeros((1, 2, 5), np.uint64)
    g.mc_batch_list(3, 0, n, 1, [1.0, 2.0], [1], np.ones((1, 2), np.uint8), ls)
    s0 = _mc(g, n, 0, [1.0, 2.0], seed=3)
    assert s0[:, F.RUN].tolist() == [n, n] and s0[:, F.DECODES].tolist() == [n, n] and (s0[:, F.FLIPPED] == 0).all()
    assert s0[:, F.ERR].tolist() == ls[0, :, 1].tolist() and s0[:, F.UNDET].tolist() == ls[0, :, 3].tolist()
    stats = np.full((3, 6), 5, np.uint64)                                  # (the call ADDS)
    g.mc_batch_flip(3, 0, n, 1, [1.0, 2.0, 3.0], 8, np.array([1, 0, 1], np.uint8), stats)
    assert (stats[1] == 5).all()
    assert (stats[0] - 5).tolist() == _mc(g, n, 8, [1.0], seed=3)[0].tolist()
    assert (stats[2] - 5).tolist() == _mc(g, n, 8, [3.0], seed=3)[0].tolist()
    assert stats[0, F.ERR] > stats[2, F.ERR] and stats[0, F.FIRST] < stats[2, F.FIRST]
    # retries never turn a first-pass word away, and help
    s8 = _mc(g, n, 8, [1.0, 2.0], seed=3)
    assert (s8[:, F.FIRST] == s0[:, F.FIRST]).all() and (s8[:, F.ERR] < s0[:, F.ERR]).all()
    # flip_stats: stops like list_stats, shares add up
    r = g.flip_stats([0.0, 6.0], 8, max_runs=200, max_err=30, seed=1, batch=64)
    st = r["stats"]
    assert (st[:, F.RUN] <= 200).all() and st[1, F.RUN] == 200 and st[1, F.ERR] <= 30 and st[0, F.ERR] > 30 and st[0, F.RUN] < 200
    assert st[0].tolist() == _mc(g, int(st[0, F.RUN]), 8, [0.0])[0].tolist()
    run = st[:, F.RUN].astype(np.float64)
    failed = (st[:, F.RUN] - st[:, F.FIRST] - st[:, F.FLIPPED]) / run
    assert np.allclose(r["first_share"] + r["flipped_share"] + failed, 1.0, rtol=1e-14)
    assert (r["bler"] == st[:, F.ERR] / run).all() and (r["undetected_rate"] == st[:, F.UNDET] / run).all()
    assert (r["mean_decodes"] == st[:, F.DECODES] / run).all() and (r["mean_decodes"] >= 1).all() and (r["mean_decodes"] <= 9).all()
    assert r["mean_decodes"][1] < r["mean_decodes"][0]


def test_sweep_bicm(built_lib, oracle_built):
    """One BICM constellation: the counters of the sweep equal those of the delivered words of a device decode of the same trials."""
    import polar_amd
    import torch
    _, g = _pair(8, 128, 8)
    n, T, snr, K = 256, 8, 4.5, 128
    got = _mc(g, n, T, [snr], constellation=polar_amd.ASK4_GRAY, seed=4)[0]
    t = torch.empty((n, 256), dtype=torch.float64, device="cuda")
    sent = torch.empty((n, K), dtype=torch.uint8, device="cuda")
    g.synth_bicm_llr_dev(polar_amd.ASK4_GRAY, 4, 0, n, snr, t.data_ptr(), sent.data_ptr())
    out, ok, nd = (x[:n] for x in _dev(g, t, "f64", n, T)[:3])
    want = F.counters(dict(info=out, crc_ok=ok, n_dec=nd), sent.cpu().numpy())
    print("bicm", got.tolist(), want.tolist())
    assert got.tolist() == want.tolist()
    assert got[F.RUN] == n and 0 < got[F.FIRST] < n and got[F.FLIPPED] > 0
    assert (_mc(g, n, T, [snr], constellation="ask4-gray", seed=4)[0] == got).all()


# ---- 9. the C++ mirror ------------------------------------------------------------------------------------------------------------
CPP_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "PolarCode.hpp"
int main(int argc, char **argv) {
    // argv[1]: file of doubles, B rows of 64; prints per codeword crc_ok, n_dec, flip, the K bits, the candidates; then a sweep
    PolarCode code(6, 32, 0.32, 8);
    std::vector<double> v;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    double x;
    while (fread(&x, sizeof x, 1, f) == 1) v.push_back(x);
    fclose(f);
    PolarCode::FlipResult r = code.decode_sc_flip(v, 4);
    for (long b = 0; b < r.B; ++b) {
        printf("%d %d %d ", (int)r.crc_ok[b], (int)r.n_dec[b], (int)r.flip[b]);
        for (int k = 0; k < r.K; ++k) putchar('0' + r.out[(size_t)b * r.K + k]);
        for (int t = 0; t < 4; ++t) {
            unsigned long long bits;
            memcpy(&bits, &r.mag[(size_t)b * 4 + t], 8);
            printf(" %d %016llx", (int)r.cand[(size_t)b * 4 + t], bits);
        }
        putchar('\n');
    }
    PolarCode::FlipStats s = code.flip_stats({1.0, 2.0}, 4, 300, 25, 7, 100);
    for (size_t i = 0; i < s.stats.size(); ++i) printf("%llu\n", (unsigned long long)s.stats[i]);
    for (int i = 0; i < s.n_points; ++i)
        printf("%.17g %.17g %.17g %.17g %.17g\n", s.bler[i], s.undetected_rate[i], s.first_share[i], s.flipped_share[i], s.mean_decodes[i]);
    return 0;
}
"""


def test_cpp_mirror(built_lib, oracle_built, tmp_path):
    from polar_amd import build
    o, g = _pair(6, 32, 8)
    B, T = 24, 4
    llr, _ = o.synth_llr(13, 0, B, o.snr_sqrt_linear(1.5))
    llr.tofile(str(tmp_path / "llr.bin"))
    (tmp_path / "main.cpp").write_text(CPP_MAIN)
    exe = str(tmp_path / "flip_main")
    here = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", build.INC, "-I", os.path.join(here, "cpp"), str(tmp_path / "main.cpp"),
                           "-o", exe, "-L", here, "-lpolar_amd", "-Wl,-rpath," + here,
                           "-Wl,-rpath," + (build._torch_lib() or "/opt/rocm/lib"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path / "llr.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out, ok, nd, flip, cand, mag = g.decode_sc_flip(llr, T, return_candidates=True)
    assert len(set(nd.tolist())) > 1
    lines = r.stdout.strip().splitlines()
    for b in range(B):
        f = lines[b].split()
        assert int(f[0]) == ok[b] and int(f[1]) == nd[b] and int(f[2]) == flip[b]
        assert f[3] == "".join(str(int(v)) for v in out[b])
        assert [int(x) for x in f[4::2]] == cand[b].tolist()
        assert [int(x, 16) for x in f[5::2]] == mag[b].view(np.uint64).tolist()
    want = g.flip_stats([1.0, 2.0], T, max_runs=300, max_err=25, seed=7, batch=100)
    assert [int(x) for x in lines[B:B + 12]] == want["stats"].reshape(-1).tolist()
    rates = np.array([[float(v) for v in l.split()] for l in lines[B + 12:]])
    assert rates.shape == (2, 5)
    for k, name in enumerate(("bler", "undetected_rate", "first_share", "flipped_share", "mean_decodes")):
        assert (rates[:, k] == want[name]).all(), name
