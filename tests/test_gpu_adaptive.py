"""Adaptive list decoding on the device (polar_decode_scl_llr_adaptive_batch[_dev], polar_mc_batch_adaptive) against the numpy model
of tests/adaptive_numpy.py, the library's own list call at every list size of the schedule, and decode_scl_llr itself."""
import os
import subprocess

import numpy as np
import pytest

import adaptive_numpy as A

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


def close(a, b):
    return abs(a - b) <= REL * max(1.0, abs(b))


def _dev_list(g, t, fmt, B, L, K):
    import torch
    cand = torch.full((B, L, K), 7, dtype=torch.uint8, device="cuda")
    pm = torch.full((B, L), -1.0, dtype=torch.float64, device="cuda")
    ok = torch.full((B, L), 7, dtype=torch.uint8, device="cuda")
    win = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    g.decode_scl_llr_list_dev(t.data_ptr(), fmt, B, L, cand.data_ptr(), pm.data_ptr(), ok.data_ptr(), 0, win.data_ptr())
    torch.cuda.synchronize()
    return cand.cpu().numpy(), pm.cpu().numpy(), ok.cpu().numpy(), win.cpu().numpy()


def _expected_from_list(g, t, fmt, B, Ls, K):
    """(out, pm, stage, crc_ok, winner of the delivering stage) from the library's list call at every list size of the schedule:
    the first stage with winner >= 0 and crc_ok[winner] == 1 delivers cand[winner], the last stage in any case."""
    out = np.zeros((B, K), np.uint8)
    pm = np.zeros(B)
    stage = np.zeros(B, np.uint8)
    ok = np.zeros(B, np.uint8)
    wins = np.zeros(B, np.int32)
    done = np.zeros(B, bool)
    rows = np.arange(B)
    for s, L in enumerate(Ls):
        cand, pm_l, ok_l, win = _dev_list(g, t, fmt, B, L, K)
        w = np.maximum(win, 0)
        acc = (win >= 0) & (ok_l[rows, w] == 1)
        take = ~done & (acc | (s == len(Ls) - 1))
        out[take] = np.where((win >= 0)[:, None], cand[rows, w], 0)[take]
        pm[take] = np.where(win >= 0, pm_l[rows, w], np.inf)[take]
        stage[take], ok[take], wins[take] = s, acc[take], win[take]
        done |= take
    assert done.all()
    return out, pm, stage, ok, wins


def _dev_adaptive(g, t, fmt, B, Ls, K, pm=True, stage=True, ok=True, stream=None):
    """The _dev call into buffers with one row of slack, filled with a sentinel: (out, pm, stage, crc_ok) as numpy arrays of B + 1
    rows (None for an output left out), after a synchronisation."""
    import torch
    bufs = _adaptive_buffers(B, K)
    _launch(g, t, fmt, B, Ls, bufs, pm, stage, ok, stream)
    torch.cuda.synchronize()
    return _fetch(bufs, pm, stage, ok)


def _adaptive_buffers(B, K):
    import torch
    return (torch.full((B + 1, K), SENT, dtype=torch.uint8, device="cuda"), torch.full((B + 1,), -1.0, dtype=torch.float64, device="cuda"),
            torch.full((B + 1,), SENT, dtype=torch.uint8, device="cuda"), torch.full((B + 1,), SENT, dtype=torch.uint8, device="cuda"))


def _launch(g, t, fmt, B, Ls, bufs, pm=True, stage=True, ok=True, stream=None):
    g.decode_scl_llr_adaptive_dev(t.data_ptr(), fmt, B, Ls, bufs[0].data_ptr(), bufs[1].data_ptr() if pm else 0,
                                  bufs[2].data_ptr() if stage else 0, bufs[3].data_ptr() if ok else 0, stream=stream)


def _fetch(bufs, pm=True, stage=True, ok=True):
    return (bufs[0].cpu().numpy(), bufs[1].cpu().numpy() if pm else None, bufs[2].cpu().numpy() if stage else None,
            bufs[3].cpu().numpy() if ok else None)


def _check_slack(got, B):
    """Every row below B is written (no sentinel left in stage / crc_ok / pm; out holds bits), the slack row is untouched."""
    out, pm, stage, ok = got
    assert (out[:B] <= 1).all() and (out[B] == SENT).all()
    if pm is not None:
        assert (pm[:B] >= 0).all() and pm[B] == -1.0
    if stage is not None:
        assert (stage[:B] != SENT).all() and stage[B] == SENT
    if ok is not None:
        assert (ok[:B] <= 1).all() and ok[B] == SENT


def _same(got, want, B):
    out, pm, stage, ok = got
    assert (out[:B] == want[0]).all()
    assert (pm[:B].view(np.uint64) == want[1].view(np.uint64)).all()
    assert (stage[:B] == want[2]).all() and (ok[:B] == want[3]).all()


def _synth(g, seed, B, ebno, N, info=False):
    import torch
    t = torch.empty((B, N), dtype=torch.float64, device="cuda")
    sent = torch.empty((B, g.K), dtype=torch.uint8, device="cuda") if info else None
    g.synth_llr_dev(seed, 0, B, g.snr_sqrt_linear(ebno), t.data_ptr(), sent.data_ptr() if info else 0)
    torch.cuda.synchronize()
    return (t, sent.cpu().numpy()) if info else t


# ---- 1. against numpy on the rows of the table -------------------------------------------------------------------------------
@pytest.mark.parametrize("key,Ls,counts,errors,accepted", A.TABLE)
def test_table_rows_equal_numpy(built_lib, oracle_built, key, Ls, counts, errors, accepted):
    o, code, llr, sent, (info, pm, stage, ok) = A.reference(key, Ls)
    _, g = _pair(*key)
    out, gpm, gst, gok = g.decode_scl_llr_adaptive(llr, Ls)
    print(key, Ls, "device stages", np.bincount(gst, minlength=len(Ls)).tolist(), "numpy", counts)
    assert (out == info).all() and (gst == stage).all() and (gok == ok).all()
    assert all(close(gpm[b], pm[b]) for b in range(len(llr)))
    assert np.bincount(gst, minlength=len(Ls)).tolist() == counts
    assert int((out != sent).any(axis=1).sum()) == errors and int(gok.sum()) == accepted


# ---- 2. against the library's own list call at working shapes ------------------------------------------------------------------
# Eb/N0 chosen on the CPU with the oracle (block errors of 256 rows of seed 21 at the list sizes of the schedules: every one of
# them leaves errors for the next) so that every stage of every schedule delivers something; the test asserts it on the counts.
# The last two: an all-frozen prefix served by the prefix pass, of 255 leaves at (11, 1024, 16) — one short of the 256-leaf block
# the pass takes there, so the walk resumes INSIDE the block — and of at least 256 leaves at (11, 768, 16).
WORKING = [((10, 512, 8), (1, 2, 4, 8), 1.5), ((11, 1024, 16), (1, 4, 32), 1.25), ((11, 1024, 16), (3, 6), 1.25),
           ((11, 1024, 16), (4, 16), 1.25), ((11, 768, 16), (4, 16), 1.0)]


@pytest.mark.parametrize("key,Ls,ebno", WORKING)
def test_working_shapes_equal_the_list_call(built_lib, oracle_built, key, Ls, ebno):
    import torch
    n, K, crc = key
    _, g = _pair(n, K, crc)
    B, N = 256, 1 << n
    if Ls == (4, 16):
        prefix = int(np.argmin(g.frozen_bits))            # first unfrozen leaf = length of the all-frozen prefix
        assert (prefix >= 256) if K == 768 else (prefix == 255), prefix
    t = _synth(g, 21, B, ebno, N)
    want = _expected_from_list(g, t, "f64", B, Ls, K)
    counts = np.bincount(want[2], minlength=len(Ls)).tolist()
    print(key, Ls, ebno, "stages", counts, "accepted", int(want[3].sum()))
    assert min(counts) > 0, counts
    assert (want[4] == 0).all()                            # (no degenerate row here: the winner is row 0 of its list)
    got = _dev_adaptive(g, t, "f64", B, Ls, K)
    _check_slack(got, B)
    _same(got, want, B)
    assert (got[3][:B][got[2][:B] < len(Ls) - 1] == 1).all()
    # out == decode_scl_llr(row, Ls[s*]) in automatic mode and with the LLR-domain kernels
    out = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    try:
        for mode in (0, 1):
            g.set_mode(mode)
            for s, L in enumerate(Ls):
                g.decode_scl_llr_dev(t.data_ptr(), B, L, out.data_ptr())
                torch.cuda.synchronize()
                sel = got[2][:B] == s
                assert (out.cpu().numpy()[sel] == got[0][:B][sel]).all(), (mode, s, L)
    finally:
        g.set_mode(0)


# ---- 3. work-list edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 63, 65, 257])
def test_work_list_edges(built_lib, oracle_built, B):
    """(6, 32, 8) under (1, 2, 4, 8): 64, 32, 16 and 8 codewords per wave, so every stage has a partial last group. Expected values
    from the library's list call (checked against numpy by test_gpu_scl_list.py), not from the numpy model: at -10 dB scl_list
    meets ties it does not restate. 8 dB: everything is delivered by stage 0 and the later launches see empty lists; -10 dB: nearly
    everything reaches the last stage; 1.5 dB: every stage works."""
    _, g = _pair(6, 32, 8)
    Ls, K = (1, 2, 4, 8), 32
    for ebno in (8.0, -10.0, 1.5):
        t = _synth(g, 30 + B, B, ebno, 64)
        want = _expected_from_list(g, t, "f64", B, Ls, K)
        got = _dev_adaptive(g, t, "f64", B, Ls, K)
        _check_slack(got, B)
        _same(got, want, B)
        counts = np.bincount(got[2][:B], minlength=4)
        print(B, ebno, counts.tolist())
        if ebno == 8.0:
            assert counts[0] == B and (got[3][:B] == 1).all()
        elif ebno == -10.0 and B >= 63:
            assert counts[3] > 0.8 * B
        elif ebno == 1.5 and B >= 257:
            assert counts.min() > 0


# ---- 4. optional outputs ----------------------------------------------------------------------------------------------------------
def test_optional_outputs(built_lib, oracle_built):
    _, g = _pair(6, 32, 8)
    B, Ls, K = 65, (1, 2, 4, 8), 32
    t = _synth(g, 41, B, 1.5, 64)
    full = _dev_adaptive(g, t, "f64", B, Ls, K)
    _check_slack(full, B)
    for pm, stage, ok in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        got = _dev_adaptive(g, t, "f64", B, Ls, K, pm=pm, stage=stage, ok=ok)
        _check_slack(got, B)
        for a, b in zip(got, full):
            assert a is None or a.tobytes() == b.tobytes(), (pm, stage, ok)


# ---- 5. two calls on one stream, no synchronisation between them -------------------------------------------------------------------
def test_two_calls_on_one_stream(built_lib, oracle_built):
    import torch
    _, g = _pair(6, 32, 8)
    K = 32
    (B1, Ls1), (B2, Ls2) = (257, (1, 8)), (65, (2, 4, 8))
    t1, t2 = _synth(g, 51, B1, 1.0, 64), _synth(g, 52, B2, 0.5, 64)
    want1, want2 = _expected_from_list(g, t1, "f64", B1, Ls1, K), _expected_from_list(g, t2, "f64", B2, Ls2, K)
    assert min(np.bincount(want1[2], minlength=2)) > 0 and min(np.bincount(want2[2], minlength=3)) > 0
    # (a first pair of calls sizes the handle's scratch: the pair under test then allocates nothing, so nothing synchronises)
    _dev_adaptive(g, t1, "f64", B1, Ls1, K)
    _dev_adaptive(g, t2, "f64", B2, Ls2, K)
    st = torch.cuda.Stream()
    b1, b2 = _adaptive_buffers(B1, K), _adaptive_buffers(B2, K)
    torch.cuda.synchronize()
    allocs = g.debug_get("allocs")
    with torch.cuda.stream(st):
        _launch(g, t1, "f64", B1, Ls1, b1, stream=st)
        _launch(g, t2, "f64", B2, Ls2, b2, stream=st)
    assert g.debug_get("allocs") == allocs
    torch.cuda.synchronize()
    got1, got2 = _fetch(b1), _fetch(b2)
    _check_slack(got1, B1)
    _check_slack(got2, B2)
    _same(got1, want1, B1)
    _same(got2, want2, B2)


# ---- 6. element formats, host form ------------------------------------------------------------------------------------------------
def test_formats_and_host_form(built_lib, oracle_built):
    import torch
    from llr16_util import to_bf16_patterns, widen_bf16
    o, g = _pair(6, 32, 8)
    B, Ls, K = 65, (1, 2, 4, 8), 32
    llr, _ = o.synth_llr(9, 0, B, o.snr_sqrt_linear(1.5))
    f32 = llr.astype(np.float32)
    f16 = llr.astype(np.float16)
    b16 = to_bf16_patterns(llr)
    for fmt, rows, wide in (("f64", llr, llr), ("f32", f32, f32.astype(np.float64)), ("f16", f16, f16.astype(np.float64)),
                            ("bf16", b16, widen_bf16(b16))):
        want = _dev_adaptive(g, torch.tensor(wide, device="cuda"), "f64", B, Ls, K)
        src = torch.tensor(rows.view(np.int16) if rows.dtype.itemsize == 2 else rows, device="cuda")
        got = _dev_adaptive(g, src, fmt, B, Ls, K)
        _check_slack(got, B)
        host = g.decode_scl_llr_adaptive(rows, Ls, fmt=fmt if fmt == "bf16" else None)
        for w, a, h in zip(want, got, host):
            assert w.tobytes() == a.tobytes() and w[:B].tobytes() == h.tobytes(), fmt
        assert len(set(got[2][:B].tolist())) > 1, fmt
    # the host form with outputs left out, called through the C-ABI
    import ctypes as C
    out = np.zeros((B, K), np.uint8)
    a = np.array(Ls, np.uint8)
    assert g._L.polar_decode_scl_llr_adaptive_batch(g._h, C.c_void_p(llr.ctypes.data), C.c_int(0), C.c_long(B), C.c_void_p(a.ctypes.data),
                                                    C.c_int(len(Ls)), C.c_void_p(out.ctypes.data), None, None, None) == 0
    assert (out == g.decode_scl_llr_adaptive(llr, Ls)[0]).all()


# ---- 7. the degenerate rows -------------------------------------------------------------------------------------------------------
def test_degenerate_rows(built_lib, oracle_built):
    """The rows of test_degenerate_rows (tests/test_gpu_scl_list.py) on a code with a check bit: every path meets a frozen leaf whose
    cost is +inf, and a list of 16 or more never fills (3 unfrozen leaves: 8 paths) — no winner row, winner -1."""
    import torch
    _, g = _pair(4, 2, 1)
    K = 2
    llr = np.zeros((4, 16))
    llr[0] = np.where(np.arange(16) % 2 == 0, 1e3, -1e3)
    llr[1], llr[2], llr[3] = 0.5 * llr[0], 0.7 * llr[0], 0.8 * llr[0]
    t = torch.tensor(llr, device="cuda")
    for Ls in ((16,), (64,), (16, 64), (1, 2, 16, 64)):
        want = _expected_from_list(g, t, "f64", 4, Ls, K)
        lost = want[4] == -1
        # (a row without a winner at 16 is not accepted there and has none at 64 either; behind a list of 1 or 2, which always fills,
        # a row may be delivered earlier: that schedule is compared, not counted)
        assert lost.any() or Ls[0] < 16, Ls
        got = _dev_adaptive(g, t, "f64", 4, Ls, K)
        out, pm, stage, ok = (x[:4] for x in got)
        assert (out == want[0]).all() and (stage == want[2]).all() and (ok == want[3]).all()
        assert (stage[lost] == len(Ls) - 1).all() and (ok[lost] == 0).all() and (out[lost] == 0).all() and np.isposinf(pm[lost]).all()
        assert (pm[~lost].view(np.uint64) == want[1][~lost].view(np.uint64)).all()
        assert (got[0][4] == SENT).all()
        host = g.decode_scl_llr_adaptive(llr, Ls)
        assert (host[0] == out).all() and (host[2] == stage).all() and (host[3] == ok).all()


# ---- 8. the sweep ---------------------------------------------------------------------------------------------------------------
def _mc(g, T, Ls, axis, enabled=None, t0=0, stride=1, constellation=0, seed=1):
    stats = np.zeros((len(axis), 3 + len(Ls)), np.uint64)
    g.mc_batch_adaptive(seed, t0, T, stride, axis, Ls, np.ones(len(axis), np.uint8) if enabled is None else enabled, stats, constellation)
    return stats


@pytest.mark.parametrize("key,Ls,counts,errors,accepted", A.TABLE)
def test_sweep_counters_equal_numpy(built_lib, oracle_built, key, Ls, counts, errors, accepted):
    import list_stats_numpy as LS
    o, code, llr, sent, (info, pm, stage, ok) = A.reference(key, Ls)
    want = A.counters(info, stage, ok, sent, len(Ls))
    _, g = _pair(*key)
    T = 256
    got = _mc(g, T, Ls, [LS.STATS_EBNO], seed=LS.STATS_SEED)[0]
    print(key, Ls, "device", got.tolist(), "numpy", want.tolist())
    assert got.tolist() == want.tolist()
    assert got[A.RUN] == T and got[A.ERR] == errors and got[A.STAGE0:].tolist() == counts
    # chunks of 7 trials
    g.debug_set("list_chunk_cw", 7)
    try:
        assert _mc(g, T, Ls, [LS.STATS_EBNO], seed=LS.STATS_SEED)[0].tolist() == got.tolist()
    finally:
        g.debug_set("list_chunk_cw", 0)
    # even and odd trials
    halves = _mc(g, T // 2, Ls, [LS.STATS_EBNO], t0=0, stride=2) + _mc(g, T // 2, Ls, [LS.STATS_EBNO], t0=1, stride=2)
    assert halves[0].tolist() == got.tolist()


def test_sweep_single_stage_points_and_a_disabled_point(built_lib, oracle_built):
    _, g = _pair(6, 32, 8)
    T = 256
    for L in (1, 3, 8):
        ls = np.zeros((1, 2, 5), np.uint64)
        g.mc_batch_list(3, 0, T, 1, [1.0, 2.0], [L], np.ones((1, 2), np.uint8), ls)
        ad = _mc(g, T, (L,), [1.0, 2.0], seed=3)
        assert ad[:, A.RUN].tolist() == [T, T] and ad[:, A.STAGE0].tolist() == [T, T]
        assert ad[:, A.ERR].tolist() == ls[0, :, 1].tolist() and ad[:, A.UNDET].tolist() == ls[0, :, 3].tolist(), L
    stats = np.full((3, 3 + 3), 5, np.uint64)                              # (the call ADDS)
    g.mc_batch_adaptive(3, 0, T, 1, [1.0, 2.0, 3.0], (1, 4, 8), np.array([1, 0, 1], np.uint8), stats)
    assert (stats[1] == 5).all()
    assert (stats[0] - 5).tolist() == _mc(g, T, (1, 4, 8), [1.0], seed=3)[0].tolist()
    assert (stats[2] - 5).tolist() == _mc(g, T, (1, 4, 8), [3.0], seed=3)[0].tolist()
    assert stats[0, A.ERR] > stats[2, A.ERR] and stats[0, A.STAGE0] < stats[2, A.STAGE0]


def test_sweep_bicm(built_lib, oracle_built):
    """One BICM constellation: the counters of the sweep equal those of the delivered words of a device decode of the same trials."""
    import polar_amd
    import torch
    _, g = _pair(8, 128, 8)
    T, Ls, snr, K = 256, (1, 4, 8), 4.5, 128
    got = _mc(g, T, Ls, [snr], constellation=polar_amd.ASK4_GRAY, seed=4)[0]
    t = torch.empty((T, 256), dtype=torch.float64, device="cuda")
    sent = torch.empty((T, K), dtype=torch.uint8, device="cuda")
    g.synth_bicm_llr_dev(polar_amd.ASK4_GRAY, 4, 0, T, snr, t.data_ptr(), sent.data_ptr())
    out, pm, stage, ok = (x[:T] for x in _dev_adaptive(g, t, "f64", T, Ls, K))
    want = A.counters(out, stage, ok, sent.cpu().numpy(), len(Ls))
    print("bicm", got.tolist(), want.tolist())
    assert got.tolist() == want.tolist()
    assert got[A.RUN] == T and got[A.STAGE0:].sum() == T and 0 < got[A.STAGE0] < T
    assert (_mc(g, T, Ls, [snr], constellation="ask4-gray", seed=4)[0] == got).all()
    ls = np.zeros((1, 1, 5), np.uint64)
    g.mc_batch_list(4, 0, T, 1, [snr], [4], np.ones((1, 1), np.uint8), ls, polar_amd.ASK4_GRAY)
    one = _mc(g, T, (4,), [snr], constellation=polar_amd.ASK4_GRAY, seed=4)[0]
    assert one[A.ERR] == ls[0, 0, 1] and one[A.UNDET] == ls[0, 0, 3]


def test_adaptive_stats_stops_and_rates(built_lib, oracle_built):
    _, g = _pair(6, 32, 8)
    # a single-stage schedule stops where list_stats stops at that list size
    r = g.adaptive_stats([1.5], (4,), max_runs=1000, max_err=20, seed=1, batch=64)
    ls = g.list_stats([1.5], [4], max_runs=1000, max_err=20, seed=1, batch=64)["stats"][0, 0]
    st = r["stats"][0]
    assert st[A.RUN] == ls[0] and st[A.ERR] == ls[1] and st[A.UNDET] == ls[3]
    assert st[A.ERR] > 20 and st[A.RUN] % 64 == 0 and 64 <= st[A.RUN] < 1000
    assert r["mean_effort"][0] == 4.0 and r["stage_share"][0, 0] == 1.0
    # max_runs is never exceeded; a point that reached max_err stops, the other goes on
    Ls = (1, 2, 8)
    r2 = g.adaptive_stats([0.0, 6.0], Ls, max_runs=200, max_err=30, seed=1, batch=64)
    s2 = r2["stats"]
    assert (s2[:, A.RUN] <= 200).all() and s2[1, A.RUN] == 200 and s2[1, A.ERR] <= 30
    assert s2[0, A.ERR] > 30 and s2[0, A.RUN] < 200
    assert s2[0].tolist() == _mc(g, int(s2[0, A.RUN]), Ls, [0.0])[0].tolist()
    assert (s2[:, A.STAGE0:].sum(axis=1) == s2[:, A.RUN]).all()
    run = s2[:, A.RUN].astype(np.float64)
    assert (r2["bler"] == s2[:, A.ERR] / run).all() and (r2["undetected_rate"] == s2[:, A.UNDET] / run).all()
    assert (r2["stage_share"] == s2[:, A.STAGE0:] / run[:, None]).all()
    effort = (s2[:, A.STAGE0] * 1.0 + s2[:, A.STAGE0 + 1] * 3.0 + s2[:, A.STAGE0 + 2] * 11.0) / run
    assert np.allclose(r2["mean_effort"], effort, rtol=1e-14) and 1.0 <= r2["mean_effort"][1] < r2["mean_effort"][0] <= 11.0


# ---- 9. the C++ mirror ------------------------------------------------------------------------------------------------------------
CPP_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "PolarCode.hpp"
int main(int argc, char **argv) {
    // argv[1]: file of doubles, B rows of 64; prints per codeword stage, crc_ok, the metric's bits, the K bits; then a sweep
    PolarCode code(6, 32, 0.32, 8);
    std::vector<double> v;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    double x;
    while (fread(&x, sizeof x, 1, f) == 1) v.push_back(x);
    fclose(f);
    PolarCode::AdaptiveResult r = code.decode_scl_llr_adaptive(v, {1, 3, 8});
    for (long b = 0; b < r.B; ++b) {
        unsigned long long bits;
        memcpy(&bits, &r.pm[b], 8);
        printf("%d %d %016llx ", (int)r.stage[b], (int)r.crc_ok[b], bits);
        for (int k = 0; k < r.K; ++k) putchar('0' + r.out[(size_t)b * r.K + k]);
        putchar('\n');
    }
    PolarCode::AdaptiveStats s = code.adaptive_stats({1.0, 2.0}, {1, 3, 8}, 300, 25, 7, 100);
    for (size_t i = 0; i < s.stats.size(); ++i) printf("%llu\n", (unsigned long long)s.stats[i]);
    for (int i = 0; i < s.n_points; ++i)
        printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", s.bler[i], s.undetected_rate[i], s.mean_effort[i], s.stage_share[i * 3],
               s.stage_share[i * 3 + 1], s.stage_share[i * 3 + 2]);
    return 0;
}
"""


def test_cpp_mirror(built_lib, oracle_built, tmp_path):
    from polar_amd import build
    o, g = _pair(6, 32, 8)
    B, Ls = 24, (1, 3, 8)
    llr, _ = o.synth_llr(13, 0, B, o.snr_sqrt_linear(1.5))
    llr.tofile(str(tmp_path / "llr.bin"))
    (tmp_path / "main.cpp").write_text(CPP_MAIN)
    exe = str(tmp_path / "adaptive_main")
    here = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", build.INC, "-I", os.path.join(here, "cpp"), str(tmp_path / "main.cpp"),
                           "-o", exe, "-L", here, "-lpolar_amd", "-Wl,-rpath," + here,
                           "-Wl,-rpath," + (build._torch_lib() or "/opt/rocm/lib"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path / "llr.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out, pm, stage, ok = g.decode_scl_llr_adaptive(llr, Ls)
    assert len(set(stage.tolist())) > 1
    lines = r.stdout.strip().splitlines()
    for b in range(B):
        f_stage, f_ok, f_pm, f_bits = lines[b].split()
        assert int(f_stage) == stage[b] and int(f_ok) == ok[b] and int(f_pm, 16) == int(pm[b:b + 1].view(np.uint64)[0])
        assert f_bits == "".join(str(int(v)) for v in out[b])
    want = g.adaptive_stats([1.0, 2.0], Ls, max_runs=300, max_err=25, seed=7, batch=100)
    assert [int(x) for x in lines[B:B + 12]] == want["stats"].reshape(-1).tolist()
    rates = np.array([[float(v) for v in l.split()] for l in lines[B + 12:]])
    assert rates.shape == (2, 6)
    assert (rates[:, 0] == want["bler"]).all() and (rates[:, 1] == want["undetected_rate"]).all()
    assert np.allclose(rates[:, 2], want["mean_effort"], rtol=1e-14) and (rates[:, 3:] == want["stage_share"]).all()
