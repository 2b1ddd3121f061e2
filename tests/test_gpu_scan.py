"""SCAN soft-output decoding on the device (polar_decode_scan_batch[_dev], polar_mc_batch_scan) against the numpy model of
tests/scan_numpy.py: min-sum arithmetic bit for bit on every output of every row, the first trials as they come; exact arithmetic with
the hard outputs exact and the soft ones within the CPU-measured TOL (rows scaled by 50: TOL_SCALED), on rows the model refuses none of
(scan_numpy.clean_rows)."""
import os
import subprocess

import numpy as np
import pytest

import scan_numpy as M

pytestmark = pytest.mark.gpu
SENT, FILL = 0xA5, -7.5          # sentinels of the byte and the double outputs


def _gpu(key, srand=1):
    import ctypes as C
    import polar_amd
    C.CDLL(None).srand(C.c_uint(srand))
    return polar_amd.PolarCode(key[0], key[1], 0.32, key[2])


def _same(got, r, tol=None, rows=slice(None)):
    """(out, info_llr, ext, crc_ok, n_iter) against a decode() result: hard outputs exactly; soft ones bit for bit (tol None; a zero of
    either sign is a zero) or within tol with the same +inf pattern."""
    out, info_llr, ext, ok, nit = got
    assert np.array_equal(out, r["info"][rows]) and np.array_equal(ok, r["crc_ok"][rows]) and np.array_equal(nit, r["n_iter"][rows])
    assert (out == (info_llr < 0)).all()
    if tol is None:
        assert np.array_equal(info_llr, r["info_llr"][rows]) and np.array_equal(ext, r["ext"][rows])
    else:
        assert M.same_soft(info_llr, r["info_llr"][rows], tol) and M.same_soft(ext, r["ext"][rows], tol)


def _buffers(B, K, N):
    import torch
    return (torch.full((B + 1, K), SENT, dtype=torch.uint8, device="cuda"), torch.full((B + 1, K), FILL, dtype=torch.float64, device="cuda"),
            torch.full((B + 1, N), FILL, dtype=torch.float64, device="cuda"), torch.full((B + 1,), SENT, dtype=torch.uint8, device="cuda"),
            torch.full((B + 1,), SENT, dtype=torch.uint8, device="cuda"))


def _launch(g, t, fmt, B, iters, bufs, use=(True,) * 4, minsum=False, early=False, stream=None):
    g.decode_scan_dev(t.data_ptr(), fmt, B, iters, bufs[0].data_ptr(), *[b.data_ptr() if u else 0 for b, u in zip(bufs[1:], use)],
                      minsum=minsum, early_stop=early, stream=stream)


def _fetch(bufs, use=(True,) * 4):
    return [bufs[0].cpu().numpy()] + [b.cpu().numpy() if u else None for b, u in zip(bufs[1:], use)]


def _dev(g, t, fmt, B, iters, use=(True,) * 4, minsum=False, early=False, stream=None):
    """The _dev call into sentinel-filled buffers with one row of slack: (out, info_llr, ext, crc_ok, n_iter) of B + 1 rows (None for an
    output left out), after a synchronisation."""
    import torch
    bufs = _buffers(B, g.K, g.N)
    _launch(g, t, fmt, B, iters, bufs, use, minsum, early, stream)
    torch.cuda.synchronize()
    return _fetch(bufs, use)


def _check_slack(got, B, iters):
    """Every row below B is written, the slack row is untouched."""
    out, info_llr, ext, ok, nit = got
    assert (out[:B] <= 1).all() and (out[B] == SENT).all()
    if info_llr is not None:
        assert (info_llr[:B] != FILL).all() and (info_llr[B] == FILL).all()
    if ext is not None:
        assert (ext[:B] != FILL).all() and (ext[B] == FILL).all()
    if ok is not None:
        assert (ok[:B] <= 1).all() and ok[B] == SENT
    if nit is not None:
        assert (nit[:B] >= 1).all() and (nit[:B] <= iters).all() and nit[B] == SENT


def _cases(key):
    return [(it, e) for it in M.ITERS for e in ((False, True) if key[2] else (False,))]


# ---- 1. min-sum arithmetic: bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", M.CODES)
def test_minsum_equals_numpy_bit_for_bit(built_lib, oracle_built, key):
    """The first 64 trials at 1.5 dB as they come (no margin: zeros, near-zeros and cancelling additions included), the same scaled
    by 50, the all-zero row and a row of one large value; 1, 2, 4 iterations, with and without early stop: every output of every
    row, the +inf pattern of ext included."""
    _, code = M.code_of(key)
    g = _gpu(key)
    plain = M.plain_rows(key)[0]
    llr = np.concatenate([plain, M.SCALE * plain, M.special_rows(key)])
    for it, early in _cases(key):
        r = M.decode(code, llr, it, minsum=True, early_stop=early)
        got = g.decode_scan(llr, it, minsum=True, early_stop=early)
        print(key, it, early, "n_iter", np.bincount(got[4], minlength=it + 1).tolist(), "crc_ok", int(got[3].sum()))
        _same(got, r)
        assert (got[0][-2] == 0).all() and (got[1][-2] == 0).all() and (got[2][-2][np.isfinite(got[2][-2])] == 0).all()


# ---- 2. exact arithmetic --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", M.CODES)
def test_exact_equals_numpy_within_tol(built_lib, oracle_built, key):
    """64 rows the model refuses none of, and 64 such rows scaled by 50 at every `iters` but 4 at n = 10 and 11
    (scan_numpy.scaled_iters). out, crc_ok, n_iter and the +inf pattern exactly, finite soft values within TOL (scaled rows:
    TOL_SCALED). The all-zero row: every finite output exactly 0."""
    _, code = M.code_of(key)
    g = _gpu(key)
    sets = [("plain", M.clean_rows(key)[0], M.TOL, M.MARGIN, M.ITERS),
            ("scaled", M.clean_rows(key, scale=M.SCALE)[0], M.TOL_SCALED, M.MARGIN_SCALED, M.scaled_iters(key))]
    for it, early in _cases(key):
        for name, llr, tol, margin, its in sets:
            if it not in its:
                continue
            r = M.decode(code, llr, it, early_stop=early, margin=margin)     # (raises MarginError if a row could depend on tol: none may)
            got = g.decode_scan(llr, it, early_stop=early)
            dev = max(float(np.abs(np.where(np.isfinite(w), a - np.where(np.isfinite(w), w, 0), 0)).max())
                      for a, w in ((got[1], r["info_llr"]), (got[2], r["ext"])))
            print(key, name, it, early, "largest deviation %.3g (tolerance %.3g)" % (dev, tol), "n_iter",
                  np.bincount(got[4], minlength=it + 1).tolist())
            _same(got, r, tol)
            if name == "plain" and early and it == 4 and key[0] in (5, 6, 7):
                h = np.bincount(got[4], minlength=5)
                assert h[1] > 0 and h[2] + h[3] > 0 and ((got[4] == 4) & (got[3] == 0)).sum() > 0
            if not early:
                assert (got[4] == it).all()
    z = g.decode_scan(np.zeros((1, code.N)), 4, early_stop=key[2] > 0)
    assert (z[0] == 0).all() and (z[1] == 0).all() and (z[2][np.isfinite(z[2])] == 0).all() and z[3][0] == 1
    assert z[4][0] == (1 if key[2] else 4) and not np.isnan(z[2]).any()


def test_a_frozen_tail_gives_infinite_ext(built_lib):
    """An explicit code whose frozen set fixes coded bits (scan_numpy.TailTables): ext is +inf exactly there, and a right child that
    is all frozen beside a left one that is not is pruned without changing a value."""
    import warnings
    import polar_amd
    import scl_list_numpy as S
    src = M.TailTables()
    code = S.Code(src)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", polar_amd.PolarWeakLeavesWarning)
        g = polar_amd.PolarCode.from_tables(src.n, src.K, 0, src.frozen(), src.order())
    llr = M.tail_rows()
    forced = M.forced_coded_bits(code)
    for it in M.ITERS:
        got = g.decode_scan(llr, it, minsum=True)
        _same(got, M.decode(code, llr, it, minsum=True))
        assert (np.isposinf(got[2]) == forced).all() and forced.any()
        _same(g.decode_scan(llr, it), M.decode(code, llr, it), M.TOL)


def test_n_above_the_cap_is_refused(built_lib):
    import polar_amd
    import torch
    n, K, crc = M.REFUSED
    g = polar_amd.PolarCode(n, K, 0.32, crc)
    with pytest.raises(polar_amd.PolarError, match="-4"):
        g.decode_scan(np.ones((1, 1 << n)), 2)
    t = torch.ones((1, 1 << n), dtype=torch.float64, device="cuda")
    out = torch.full((1, K), SENT, dtype=torch.uint8, device="cuda")
    with pytest.raises(polar_amd.PolarError, match="-4"):
        g.decode_scan_dev(t.data_ptr(), "f64", 1, 2, out.data_ptr())
    with pytest.raises(polar_amd.PolarError, match="-4"):
        g.mc_batch_scan(1, 0, 4, 1, [1.5], 2, np.ones(1, np.uint8), np.zeros((1, 4), np.uint64))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all()
    # a device-side refusal is an argument error as well: flags and iters are looked at before anything is launched
    g6 = _gpu((6, 32, 8))
    for kw in (dict(iters=0), dict(iters=33)):
        with pytest.raises(polar_amd.PolarError, match="-1"):
            g6.decode_scan_dev(t.data_ptr(), "f64", 1, kw["iters"], out.data_ptr())
    with pytest.raises(polar_amd.PolarError, match="-1"):
        _gpu((6, 32, 0)).decode_scan_dev(t.data_ptr(), "f64", 1, 2, out.data_ptr(), early_stop=True)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all()


# ---- 3. batch and launch geometry -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", M.EDGE_B + [M.GRID_CAP_ROWS])
def test_batch_sizes_and_the_grid_cap(built_lib, oracle_built, B):
    """(5, 16, 8): B = 1, 63, 65, 257, and one row more than the launch has blocks — the grid-stride loop runs twice in block 0 and the
    second trip starts from clean state. Both arithmetics, 4 iterations with early stop and 2 without."""
    import torch
    key = (5, 16, 8)
    _, code = M.code_of(key)
    g = _gpu(key)
    assert g.debug_get("scan_grid_cap") + 1 == M.GRID_CAP_ROWS
    llr = M.clean_rows(key, B, seed=M.EDGE_SEED + B)[0]
    t = torch.tensor(llr, device="cuda")
    for minsum in (True, False):
        for it, early in ((4, True), (2, False)):
            r = M.decode(code, llr, it, minsum=minsum, early_stop=early)
            got = _dev(g, t, "f64", B, it, minsum=minsum, early=early)
            _check_slack(got, B, it)
            _same([x[:B] for x in got], r, None if minsum else M.TOL)
    if B >= 63:
        assert len(set(r["crc_ok"].tolist())) == 2


@pytest.mark.parametrize("minsum", [True, False])
def test_a_hard_row_leaves_nothing_behind(built_lib, oracle_built, minsum):
    """The B of the right children persists across iterations and is reset per row. A batch of one row more than the launch has
    blocks, whose row 0 is a hard row (4 iterations, never passes) and whose other rows are one easy row (passes at once): block 0
    decodes the hard row and then, in its second trip, the easy row 8192. Every row equals the single-row call of its kind, byte for
    byte. Then the same with the kinds swapped."""
    import torch
    key = (7, 64, 8)
    _, code = M.code_of(key)
    g = _gpu(key)
    llr = M.clean_rows(key)[0]
    r = M.decode(code, llr, 4, minsum=minsum, early_stop=True)
    hard = np.flatnonzero((r["n_iter"] == 4) & (r["crc_ok"] == 0))
    easy = np.flatnonzero(r["n_iter"] == 1)
    assert len(hard) and len(easy)
    B = M.GRID_CAP_ROWS
    assert g.debug_get("scan_grid_cap") + 1 == B
    for first, rest in ((hard[0], easy[0]), (easy[0], hard[0])):
        one_first = _dev(g, torch.tensor(llr[first:first + 1], device="cuda"), "f64", 1, 4, minsum=minsum, early=True)
        one_rest = _dev(g, torch.tensor(llr[rest:rest + 1], device="cuda"), "f64", 1, 4, minsum=minsum, early=True)
        assert one_first[4][0] != one_rest[4][0]
        big = np.repeat(llr[rest:rest + 1], B, axis=0)
        big[0] = llr[first]
        got = _dev(g, torch.tensor(big, device="cuda"), "f64", B, 4, minsum=minsum, early=True)
        _check_slack(got, B, 4)
        for a, f1, r1 in zip(got, one_first, one_rest):
            assert a[0].tobytes() == f1[0].tobytes()
            assert (a[1:B].reshape(B - 1, -1).view(np.uint8) == r1[:1].reshape(1, -1).view(np.uint8)).all()


# ---- 4. outputs and stream order ------------------------------------------------------------------------------------------------------
def test_optional_outputs(built_lib, oracle_built):
    import torch
    key = (6, 32, 8)
    g = _gpu(key)
    B = 65
    t = torch.tensor(M.clean_rows(key, B, seed=41)[0], device="cuda")
    for minsum in (False, True):
        full = _dev(g, t, "f64", B, 4, minsum=minsum, early=True)
        _check_slack(full, B, 4)
        assert len(set(full[4][:B].tolist())) > 1
        for skip in list(range(4)) + [None]:
            use = tuple(False if skip is None else k != skip for k in range(4))
            got = _dev(g, t, "f64", B, 4, use=use, minsum=minsum, early=True)
            _check_slack(got, B, 4)
            for a, b in zip(got, full):
                assert a is None or a.tobytes() == b.tobytes(), skip


def test_two_calls_on_one_stream(built_lib, oracle_built):
    import torch
    key = (6, 32, 8)
    g = _gpu(key)
    (B1, it1), (B2, it2) = (257, 4), (65, 2)
    t1 = torch.tensor(M.clean_rows(key, B1, seed=51)[0], device="cuda")
    t2 = torch.tensor(M.clean_rows(key, B2, seed=52)[0], device="cuda")
    want1 = _dev(g, t1, "f64", B1, it1, early=True)                  # (the first call uploads the schedule: nothing allocates below)
    want2 = _dev(g, t2, "f64", B2, it2, minsum=True)
    st = torch.cuda.Stream()
    b1, b2 = _buffers(B1, g.K, g.N), _buffers(B2, g.K, g.N)
    torch.cuda.synchronize()
    allocs = g.debug_get("allocs")
    with torch.cuda.stream(st):
        _launch(g, t1, "f64", B1, it1, b1, early=True, stream=st)
        _launch(g, t2, "f64", B2, it2, b2, minsum=True, stream=st)
    assert g.debug_get("allocs") == allocs
    torch.cuda.synchronize()
    for got, want in ((_fetch(b1), want1), (_fetch(b2), want2)):
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()
    _check_slack(_fetch(b1), B1, it1)
    _check_slack(_fetch(b2), B2, it2)


def test_formats_and_host_form(built_lib, oracle_built):
    """The four element formats: the model applied to the widened values (min-sum: bit for bit); the device on the narrow rows equals
    the device on the widened doubles byte for byte in both arithmetics; the host form equals the device form."""
    import torch
    from llr16_util import to_bf16_patterns, widen_bf16
    key = (6, 32, 8)
    _, code = M.code_of(key)
    g = _gpu(key)
    B = 65
    llr = M.clean_rows(key, B, seed=9)[0]
    f32, f16, b16 = llr.astype(np.float32), llr.astype(np.float16), to_bf16_patterns(llr)
    for fmt, rows, wide in (("f64", llr, llr), ("f32", f32, f32.astype(np.float64)), ("f16", f16, f16.astype(np.float64)),
                            ("bf16", b16, widen_bf16(b16))):
        src = torch.tensor(rows.view(np.int16) if rows.dtype.itemsize == 2 else rows, device="cuda")
        for minsum in (True, False):
            want = _dev(g, torch.tensor(wide, device="cuda"), "f64", B, 4, minsum=minsum, early=True)
            got = _dev(g, src, fmt, B, 4, minsum=minsum, early=True)
            _check_slack(got, B, 4)
            host = g.decode_scan(rows, 4, fmt=fmt if fmt == "bf16" else None, minsum=minsum, early_stop=True)
            for w, a, h in zip(want, got, host):
                assert w.tobytes() == a.tobytes() and w[:B].tobytes() == h.tobytes(), fmt
            if minsum:
                _same(host, M.decode(code, wide, 4, minsum=True, early_stop=True))
        assert len(set(got[4][:B].tolist())) > 1, fmt
    # the host form with outputs left out, called through the C-ABI, and a single row
    import ctypes as C
    out = np.zeros((B, g.K), np.uint8)
    assert g._L.polar_decode_scan_batch(g._h, C.c_void_p(llr.ctypes.data), C.c_int(0), C.c_long(B), C.c_int(4), C.c_int(0),
                                        C.c_void_p(out.ctypes.data), None, None, None, None) == 0
    five = g.decode_scan(llr, 4)
    assert len(five) == 5 and (out == five[0]).all()
    one = g.decode_scan(llr[0], 4)
    assert (one[0] == five[0][:1]).all() and one[1].tobytes() == five[1][:1].tobytes() and one[2].tobytes() == five[2][:1].tobytes()


# ---- 5. the sweep -----------------------------------------------------------------------------------------------------------------------
def _mc(g, T, iters, axis, enabled=None, t0=0, stride=1, constellation=0, seed=1, minsum=False, early=False):
    stats = np.zeros((len(axis), 4), np.uint64)
    g.mc_batch_scan(seed, t0, T, stride, axis, iters, np.ones(len(axis), np.uint8) if enabled is None else enabled, stats, minsum, early,
                    constellation)
    return stats


@pytest.mark.parametrize("key,iters,err,undet,it_sum,err_e,undet_e", M.TABLE)
def test_sweep_counters_equal_numpy(built_lib, oracle_built, key, iters, err, undet, it_sum, err_e, undet_e):
    import list_stats_numpy as LS
    code, llr, sent, r = M.table_reference(key, iters)
    g = _gpu(key)
    n = 256
    got = _mc(g, n, iters, [LS.STATS_EBNO], seed=LS.STATS_SEED)[0]
    got_e = _mc(g, n, iters, [LS.STATS_EBNO], seed=LS.STATS_SEED, early=True)[0]
    print(key, iters, "device", got.tolist(), got_e.tolist(), "numpy", M.counters(r, sent, key[2]).tolist())
    assert got.tolist() == M.counters(r, sent, key[2]).tolist() == [256, err, undet, 256 * iters]
    assert got_e.tolist() == [256, err_e, undet_e, it_sum]
    ms = M.decode(code, llr, iters, minsum=True, early_stop=True)
    assert _mc(g, n, iters, [LS.STATS_EBNO], seed=LS.STATS_SEED, minsum=True, early=True)[0].tolist() == M.counters(ms, sent, key[2]).tolist()
    # chunks of 7 trials
    g.debug_set("list_chunk_cw", 7)
    try:
        assert _mc(g, n, iters, [LS.STATS_EBNO], seed=LS.STATS_SEED, early=True)[0].tolist() == got_e.tolist()
    finally:
        g.debug_set("list_chunk_cw", 0)
    # even and odd trials
    halves = _mc(g, n // 2, iters, [LS.STATS_EBNO], t0=0, stride=2, early=True) + _mc(g, n // 2, iters, [LS.STATS_EBNO], t0=1, stride=2, early=True)
    assert halves[0].tolist() == got_e.tolist()


def test_sweep_a_disabled_point_bicm_mlc_and_scan_stats(built_lib, oracle_built):
    import polar_amd
    import torch
    g = _gpu((6, 32, 8))
    n = 256
    stats = np.full((3, 4), 5, np.uint64)                                  # (the call ADDS)
    g.mc_batch_scan(3, 0, n, 1, [1.0, 2.0, 3.0], 2, np.array([1, 0, 1], np.uint8), stats, early_stop=True)
    assert (stats[1] == 5).all()
    assert (stats[0] - 5).tolist() == _mc(g, n, 2, [1.0], seed=3, early=True)[0].tolist()
    assert (stats[2] - 5).tolist() == _mc(g, n, 2, [3.0], seed=3, early=True)[0].tolist()
    assert stats[0, M.ERR] > stats[2, M.ERR] and stats[0, M.ITERS_COL] > stats[2, M.ITERS_COL]
    # a code without a CRC: UNDET stays 0, ITERS = iters per trial
    g0 = _gpu((6, 32, 0))
    s0 = _mc(g0, n, 2, [1.0], seed=3)[0]
    assert s0[M.RUN] == n and s0[M.UNDET] == 0 and s0[M.ITERS_COL] == 2 * n and s0[M.ERR] > 0
    # one BICM constellation on the SNR axis: the counters equal those of a device decode of the same trials
    g8 = _gpu((8, 128, 8))
    snr, K = 4.5, 128
    got = _mc(g8, n, 4, [snr], constellation=polar_amd.ASK4_GRAY, seed=4, early=True)[0]
    t = torch.empty((n, 256), dtype=torch.float64, device="cuda")
    sent = torch.empty((n, K), dtype=torch.uint8, device="cuda")
    g8.synth_bicm_llr_dev(polar_amd.ASK4_GRAY, 4, 0, n, snr, t.data_ptr(), sent.data_ptr())
    d = _dev(g8, t, "f64", n, 4, early=True)
    want = M.counters(dict(info=d[0][:n], crc_ok=d[3][:n], n_iter=d[4][:n]), sent.cpu().numpy(), 8)
    print("bicm", got.tolist(), want.tolist())
    assert got.tolist() == want.tolist() and got[M.RUN] == n and 0 < got[M.ERR] < n and n < got[M.ITERS_COL] < 4 * n
    assert (_mc(g8, n, 4, [snr], constellation="ask4-gray", seed=4, early=True)[0] == got).all()
    with pytest.raises(polar_amd.PolarError, match="-1"):
        _mc(g8, n, 4, [snr], constellation=polar_amd.RX_MLC | polar_amd.ASK4_SP)
    # scan_stats: rounds of mc_batch_scan, stopped like list_stats
    r = g.scan_stats([0.0, 6.0], 4, max_runs=200, max_err=30, seed=1, batch=64, early_stop=True)
    st = r["stats"]
    assert (st[:, M.RUN] <= 200).all() and st[1, M.RUN] == 200 and st[1, M.ERR] <= 30 and st[0, M.ERR] > 30 and st[0, M.RUN] < 200
    assert st[0].tolist() == _mc(g, int(st[0, M.RUN]), 4, [0.0], early=True)[0].tolist()
    assert st[1].tolist() == _mc(g, 200, 4, [6.0], early=True)[0].tolist()
    run = st[:, M.RUN].astype(np.float64)
    assert (r["bler"] == st[:, M.ERR] / run).all() and (r["undetected_rate"] == st[:, M.UNDET] / run).all()
    assert (r["mean_iters"] == st[:, M.ITERS_COL] / run).all() and (r["mean_iters"] >= 1).all() and r["mean_iters"][1] < r["mean_iters"][0] <= 4


# ---- 6. the C++ mirror ------------------------------------------------------------------------------------------------------------------
CPP_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "PolarCode.hpp"
static void hex(double v) { unsigned long long b; memcpy(&b, &v, 8); printf(" %016llx", b); }
int main(int argc, char **argv) {
    // argv[1]: file of doubles, B rows of 64; prints per codeword crc_ok, n_iter, the K bits, info_llr and ext as bit patterns; then a sweep
    PolarCode code(6, 32, 0.32, 8);
    std::vector<double> v;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    double x;
    while (fread(&x, sizeof x, 1, f) == 1) v.push_back(x);
    fclose(f);
    PolarCode::ScanResult r = code.decode_scan(v, 4, POLAR_SCAN_EARLY_STOP);
    for (long b = 0; b < r.B; ++b) {
        printf("%d %d ", (int)r.crc_ok[b], (int)r.n_iter[b]);
        for (int k = 0; k < r.K; ++k) putchar('0' + r.out[(size_t)b * r.K + k]);
        for (int k = 0; k < r.K; ++k) hex(r.info_llr[(size_t)b * r.K + k]);
        for (int k = 0; k < r.N; ++k) hex(r.ext[(size_t)b * r.N + k]);
        putchar('\n');
    }
    PolarCode::ScanStats s = code.scan_stats({1.0, 2.0}, 4, POLAR_SCAN_EARLY_STOP, 300, 25, 7, 100);
    for (size_t i = 0; i < s.stats.size(); ++i) printf("%llu\n", (unsigned long long)s.stats[i]);
    for (int i = 0; i < s.n_points; ++i) printf("%.17g %.17g %.17g\n", s.bler[i], s.undetected_rate[i], s.mean_iters[i]);
    return 0;
}
"""


def test_cpp_mirror(built_lib, oracle_built, tmp_path):
    from polar_amd import build
    key = (6, 32, 8)
    g = _gpu(key)
    B = 24
    llr = M.clean_rows(key, B, seed=13)[0]
    llr.tofile(str(tmp_path / "llr.bin"))
    (tmp_path / "main.cpp").write_text(CPP_MAIN)
    exe = str(tmp_path / "scan_main")
    here = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", build.INC, "-I", os.path.join(here, "cpp"), str(tmp_path / "main.cpp"),
                           "-o", exe, "-L", here, "-lpolar_amd", "-Wl,-rpath," + here,
                           "-Wl,-rpath," + (build._torch_lib() or "/opt/rocm/lib"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path / "llr.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out, info_llr, ext, ok, nit = g.decode_scan(llr, 4, early_stop=True)
    assert len(set(nit.tolist())) > 1
    lines = r.stdout.strip().splitlines()
    for b in range(B):
        f = lines[b].split()
        assert int(f[0]) == ok[b] and int(f[1]) == nit[b] and f[2] == "".join(str(int(v)) for v in out[b])
        assert [int(x, 16) for x in f[3:3 + 32]] == info_llr[b].view(np.uint64).tolist()
        assert [int(x, 16) for x in f[3 + 32:]] == ext[b].view(np.uint64).tolist()
    want = g.scan_stats([1.0, 2.0], 4, max_runs=300, max_err=25, seed=7, batch=100, early_stop=True)
    assert [int(x) for x in lines[B:B + 8]] == want["stats"].reshape(-1).tolist()
    rates = np.array([[float(v) for v in l.split()] for l in lines[B + 8:]])
    assert rates.shape == (2, 3)
    for k, name in enumerate(("bler", "undetected_rate", "mean_iters")):
        assert (rates[:, k] == want[name]).all(), name
