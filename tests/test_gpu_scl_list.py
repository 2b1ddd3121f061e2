"""List output of decode_scl_llr on the device (polar_decode_scl_llr_list_batch[_dev], polar_list_find_dev) against the numpy list
decoder of tests/scl_list_numpy.py, the forced SC pass, and decode_scl_llr itself."""
import os
import subprocess

import numpy as np
import pytest

import scl_list_numpy as S

pytestmark = pytest.mark.gpu
REL = 1e-10          # libm against the kernel's table-driven exp / log1p: the tolerance of test_winning_path_metric_matches_oracle


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
    """The _dev call on a device tensor of rows: the five outputs as numpy arrays."""
    import torch
    cand = torch.full((B, L, K), 7, dtype=torch.uint8, device="cuda")
    pm = torch.full((B, L), -1.0, dtype=torch.float64, device="cuda")
    ok = torch.full((B, L), 7, dtype=torch.uint8, device="cuda")
    na = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    win = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    g.decode_scl_llr_list_dev(t.data_ptr(), fmt, B, L, cand.data_ptr(), pm.data_ptr(), ok.data_ptr(), na.data_ptr(), win.data_ptr())
    torch.cuda.synchronize()
    return cand.cpu().numpy(), pm.cpu().numpy(), ok.cpu().numpy(), na.cpu().numpy(), win.cpu().numpy()


def _check_order_and_padding(cand, pm, ok, na, L):
    """Rows in the specified order (CRC pass first, then the metric ascending) and the padding behind n_active."""
    for b in range(cand.shape[0]):
        a = int(na[b])
        assert 1 <= a <= L
        assert set(ok[b, :a].tolist()) <= {0, 1}
        keys = [(1 - int(ok[b, r]), pm[b, r]) for r in range(a)]
        assert keys == sorted(keys), (b, keys)
        assert (cand[b, a:] == 0).all() and (ok[b, a:] == 0).all() and np.isposinf(pm[b, a:]).all(), b


_numpy_lists = {}


def _survivors(case, L):
    """scl_list of the shared inputs, computed once per (code, list size)."""
    key = (case[:3], L)
    if key not in _numpy_lists:
        o, g = _pair(*case[:3])
        code = S.Code(o)
        llr, info = S.list_inputs(o)
        _numpy_lists[key] = (o, g, code, llr, info, [S.scl_list(code, llr[i], L) for i in range(S.LIST_ROWS)])
    return _numpy_lists[key]


@pytest.mark.parametrize("case,L", [(c, c[3]) for c in S.LIST_CASES] + [(S.LIST_CASES[0], 3), (S.LIST_CASES[0], 6), (S.LIST_CASES[0], 1)])
def test_whole_list_parity(built_lib, oracle_built, case, L):
    o, g, code, llr, _, rows = _survivors(case, L)
    cand, pm, ok, na, win = g.decode_scl_llr_list(llr, L)
    _check_order_and_padding(cand, pm, ok, na, L)
    for b in range(S.LIST_ROWS):
        a = int(na[b])
        # (with a CRC two survivors may share their K info bits and differ in the check bits they decided: the metrics of a
        # (bits, flag) pair are then compared as sorted lists)
        want, got = {}, {}
        for r in rows[b]:
            want.setdefault((r["info"].tobytes(), int(r["crc_ok"])), []).append(r["pm"])
        for r in range(a):
            got.setdefault((cand[b, r].tobytes(), int(ok[b, r])), []).append(pm[b, r])
        assert a == len(rows[b])
        assert set(got) == set(want), b
        for k in got:
            assert len(got[k]) == len(want[k]), (b, k)
            for x, y in zip(sorted(got[k]), sorted(want[k])):
                assert close(x, y), (b, x, y)
        # (no ties, so the order is the numpy order row for row)
        assert [r["info"].tobytes() for r in rows[b]] == [cand[b, r].tobytes() for r in range(a)], b
        assert win[b] == 0
    assert (cand[:, 0] == g.decode_scl_llr(llr, L)).all()


def test_exhaustive_list(built_lib, oracle_built):
    """n = 4, K = 4, no CRC: a list of 16 holds all 16 words, a list of 64 never fills."""
    o, g = _pair(4, 4, 0)
    code = S.Code(o)
    B = 32
    llr, _ = o.synth_llr(5, 0, B, o.snr_sqrt_linear(1.5))
    allw = np.array([[(w >> j) & 1 for j in range(4)] for w in range(16)], np.uint8)
    forced = np.stack([S.forced_path_metric(code, llr[b], S.word(code, allw)) for b in range(B)])
    for L in (16, 64):
        cand, pm, ok, na, win = g.decode_scl_llr_list(llr, L)
        assert (na == 16).all() and (win == 0).all()
        _check_order_and_padding(cand, pm, ok, na, L)
        for b in range(B):
            ids = [int(sum(int(cand[b, r, j]) << j for j in range(4))) for r in range(16)]
            assert sorted(ids) == list(range(16)), b
            for r in range(16):
                assert ok[b, r] == 1 and close(pm[b, r], forced[b, ids[r]]), (b, r)
            assert (np.diff(pm[b, :16]) >= 0).all()
        assert (cand[:, 0] == o.decode_scl_llr(llr, L)).all()


@pytest.mark.parametrize("n,K,crc,L", [(10, 512, 8, 8), (11, 1024, 16, 32), (9, 256, 0, 2)])
def test_winner_contract_at_working_shapes(built_lib, oracle_built, n, K, crc, L):
    """HBM-resident layers and the prefix kernel. The K bits of a row do not hold its CRC decisions, so the CRC flag and the metric
    are checked together: the forced pass along the row's bits completed with the CRC MATRIX's check bits gives the row's metric
    if and only if the row is flagged as passing (a failing row decided other check bits: a different path, a different
    metric)."""
    import torch
    o, g = _pair(n, K, crc)
    code = S.Code(o)
    B = 24
    llr, _ = o.synth_llr(808, 0, B, o.snr_sqrt_linear(1.5))
    t = torch.tensor(llr, device="cuda")
    cand, pm, ok, na, win = _dev_list(g, t, "f64", B, L, K)
    assert (win == 0).all() and (na == L).all()
    _check_order_and_padding(cand, pm, ok, na, L)
    out = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    dpm = torch.zeros(B, dtype=torch.float64, device="cuda")
    g.debug_set("lat_max_b", -1)
    try:
        for mode in (0, 1):
            g.set_mode(mode)
            assert (g.decode_scl_llr(llr, L) == cand[:, 0]).all(), mode
            g.decode_scl_llr_dev(t.data_ptr(), B, L, out.data_ptr(), dpm.data_ptr())
            torch.cuda.synchronize()
            assert (out.cpu().numpy() == cand[:, 0]).all(), mode
            ref = dpm.cpu().numpy()
            if mode == 1:
                assert (ref.view(np.uint64) == pm[:, 0].view(np.uint64)).all()
            else:
                assert all(close(pm[b, 0], ref[b]) for b in range(B))
    finally:
        g.set_mode(0)
        g.debug_set("lat_max_b", 0)
    for b in range(B):
        assert len({cand[b, r].tobytes() for r in range(L)}) == L, b
    if crc == 0:
        assert (ok == 1).all()
    for b in range(4):
        forced = S.forced_path_metric(code, llr[b], S.word(code, cand[b]))
        for r in range(L):
            assert close(pm[b, r], forced[r]) == bool(ok[b, r]), (b, r, pm[b, r], forced[r], ok[b, r])


def test_degenerate_rows(built_lib, oracle_built):
    """The rows of test_no_finite_candidate_and_a_list_that_never_filled (tests/test_gpu_parity.py)."""
    o, g = _pair(4, 3, 0)
    llr = np.zeros((4, 16))
    llr[0] = np.where(np.arange(16) % 2 == 0, 1e3, -1e3)
    llr[1], llr[2], llr[3] = 0.5 * llr[0], 0.7 * llr[0], 0.8 * llr[0]
    for L in (1, 2, 8, 16, 64):
        cand, pm, ok, na, win = g.decode_scl_llr_list(llr, L)
        _check_order_and_padding(cand, pm, ok, na, L)
        assert ((win >= -1) & (win < na)).all()
        picked = np.stack([cand[b, win[b]] if win[b] >= 0 else np.zeros(3, np.uint8) for b in range(4)])
        want = g.decode_scl_llr(llr, L)
        assert (want == o.decode_scl_llr(llr, L)).all()
        assert (picked == want).all(), L
        if L >= 16:
            assert (win == -1).any(), L
            assert (na[win == -1] < L).all()


def test_formats_and_host_form(built_lib, oracle_built):
    import torch
    from llr16_util import to_bf16_patterns, widen_bf16
    o, g = _pair(6, 32, 8)
    B, L, K = 8, 8, 32
    llr, _ = o.synth_llr(9, 0, B, o.snr_sqrt_linear(1.5))
    f32 = llr.astype(np.float32)
    f16 = llr.astype(np.float16)
    b16 = to_bf16_patterns(llr)
    for fmt, rows, wide in (("f32", f32, f32.astype(np.float64)), ("f16", f16, f16.astype(np.float64)), ("bf16", b16, widen_bf16(b16))):
        want = _dev_list(g, torch.tensor(wide, device="cuda"), "f64", B, L, K)
        src = torch.tensor(rows.view(np.int16) if rows.dtype.itemsize == 2 else rows, device="cuda")
        got = _dev_list(g, src, fmt, B, L, K)
        host = g.decode_scl_llr_list(rows, L, fmt=fmt if fmt == "bf16" else None)
        for w, a, h in zip(want, got, host):
            assert w.tobytes() == a.tobytes() == h.tobytes(), fmt
    # the host form over its output chunks: 5 codewords per chunk, 23 rows
    B2 = 23
    llr2, _ = o.synth_llr(10, 0, B2, o.snr_sqrt_linear(1.5))
    want = _dev_list(g, torch.tensor(llr2, device="cuda"), "f64", B2, L, K)
    g.debug_set("list_chunk_cw", 5)
    try:
        host = g.decode_scl_llr_list(llr2, L)
    finally:
        g.debug_set("list_chunk_cw", 0)
    for w, h in zip(want, host):
        assert w.tobytes() == h.tobytes()
    # optional outputs left out
    cand = torch.zeros((B2, L, K), dtype=torch.uint8, device="cuda")
    g.decode_scl_llr_list_dev(torch.tensor(llr2, device="cuda").data_ptr(), "f64", B2, L, cand.data_ptr())
    torch.cuda.synchronize()
    assert (cand.cpu().numpy() == want[0]).all()


# ---- the second call allocates nothing ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,crc", [(6, 32, 8), (10, 512, 8)])          # (10, 512, 8): a prefix pass in front of the groups of 8 lanes
def test_second_call_allocates_nothing(built_lib, oracle_built, n, K, crc):
    """The list call and the metric call size every buffer before their first launch (list_prepare): the same calls again find them in
    place — no hipFree / hipMalloc, so nothing synchronises — and write the same bytes."""
    import torch
    _, g = _pair(n, K, crc)
    B, L = 9, 8
    t = torch.zeros(B * (1 << n), dtype=torch.float64, device="cuda")
    g.synth_llr_dev(S.LIST_SEED, 0, B, g.snr_sqrt_linear(S.LIST_EBNO), t.data_ptr())
    torch.cuda.synchronize()

    def calls():
        cand = torch.full((B, L, K), 7, dtype=torch.uint8, device="cuda")
        pm = torch.full((B, L), -1.0, dtype=torch.float64, device="cuda")
        ok = torch.full((B, L), 7, dtype=torch.uint8, device="cuda")
        na = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        win = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        forced = torch.full((B, L), -1.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        before = g.debug_get("allocs")
        g.decode_scl_llr_list_dev(t.data_ptr(), "f64", B, L, cand.data_ptr(), pm.data_ptr(), ok.data_ptr(), na.data_ptr(), win.data_ptr())
        g.path_metric_dev(t.data_ptr(), "f64", cand.data_ptr(), B, L, forced.data_ptr())
        moved = g.debug_get("allocs") - before
        torch.cuda.synchronize()
        return moved, [x.cpu().numpy().tobytes() for x in (cand, pm, ok, na, win, forced)]
    _, first = calls()
    moved, second = calls()
    assert moved == 0
    assert second == first
    na = np.frombuffer(first[3], np.int32)
    assert ((1 <= na) & (na <= L)).all()                                   # (the calls decoded something)


def test_list_find_dev(built_lib, oracle_built):
    import torch
    o, g = _pair(6, 32, 8)
    L, K, B = 8, 32, 48
    llr, info = o.synth_llr(11, 0, B, o.snr_sqrt_linear(1.5))
    llr[:8] = np.where(np.stack([o.encode(info[i]) for i in range(8)]) == 0, 20.0, -20.0)      # noiseless rows
    sent = info.copy()
    sent[8:16, 3] ^= 1                                                                        # one flipped bit
    t = torch.tensor(llr, device="cuda")
    cand = torch.zeros((B, L, K), dtype=torch.uint8, device="cuda")
    na = torch.zeros(B, dtype=torch.int32, device="cuda")
    g.decode_scl_llr_list_dev(t.data_ptr(), "f64", B, L, cand.data_ptr(), n_active_ptr=na.data_ptr())
    rank = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    g.list_find_dev(cand.data_ptr(), na.data_ptr(), torch.tensor(sent, device="cuda").data_ptr(), B, L, rank.data_ptr())
    torch.cuda.synchronize()
    c, a, r = cand.cpu().numpy(), na.cpu().numpy(), rank.cpu().numpy()

    def search(b):
        hits = [i for i in range(a[b]) if (c[b, i] == sent[b]).all()]
        return hits[0] if hits else L
    assert [search(b) for b in range(B)] == r.tolist()
    assert (r[:8] == 0).all()
    assert (r[16:] < L).sum() > 0 and (r[8:16] == L).sum() > 0
    # a list that never filled: the all-zero word is not found in the padding behind n_active
    o2, g2 = _pair(4, 3, 0)
    llr2, _ = o2.synth_llr(12, 0, 16, o2.snr_sqrt_linear(1.5))
    llr2 = np.abs(llr2) * np.where(np.stack([o2.encode(np.array([1, 0, 1], np.uint8))] * 16) == 0, 1.0, -1.0)   # word 101 sent, no errors
    L2 = 16
    cand2 = torch.zeros((16, L2, 3), dtype=torch.uint8, device="cuda")
    na2 = torch.zeros(16, dtype=torch.int32, device="cuda")
    g2.decode_scl_llr_list_dev(torch.tensor(llr2, device="cuda").data_ptr(), "f64", 16, L2, cand2.data_ptr(), n_active_ptr=na2.data_ptr())
    zeros = torch.zeros((16, 3), dtype=torch.uint8, device="cuda")
    rank2 = torch.zeros(16, dtype=torch.int32, device="cuda")
    g2.list_find_dev(cand2.data_ptr(), na2.data_ptr(), zeros.data_ptr(), 16, L2, rank2.data_ptr())
    # with n_active forced to 7 the rows 7 .. are never looked at, wherever the all-zero word really is
    na7 = torch.full((16,), 7, dtype=torch.int32, device="cuda")
    rank7 = torch.zeros(16, dtype=torch.int32, device="cuda")
    g2.list_find_dev(cand2.data_ptr(), na7.data_ptr(), zeros.data_ptr(), 16, L2, rank7.data_ptr())
    torch.cuda.synchronize()
    c2, a2, r2, r7 = cand2.cpu().numpy(), na2.cpu().numpy(), rank2.cpu().numpy(), rank7.cpu().numpy()
    assert (a2 == 8).all() and (c2[:, 8:] == 0).all()
    for b in range(16):
        hits = [i for i in range(8) if (c2[b, i] == 0).all()]
        assert len(hits) == 1 and r2[b] == hits[0] and r2[b] < 8
        assert r7[b] == (hits[0] if hits[0] < 7 else L2)
    # a word that is in no active row, but equals the padding: info = zeros with n_active = 0 rows to look at
    na0 = torch.zeros(16, dtype=torch.int32, device="cuda")
    g2.list_find_dev(cand2.data_ptr(), na0.data_ptr(), zeros.data_ptr(), 16, L2, rank7.data_ptr())
    torch.cuda.synchronize()
    assert (rank7.cpu().numpy() == L2).all()


CPP_MAIN = r"""
#include <cstdio>
#include <vector>
#include "PolarCode.hpp"
int main(int argc, char **argv) {
    // argv[1]: file of doubles, B rows of 64; prints per codeword n_active, winner, then per row crc_ok, the metric's bits, the K bits
    PolarCode code(6, 32, 0.32, 8);
    std::vector<double> v;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    double x;
    while (fread(&x, sizeof x, 1, f) == 1) v.push_back(x);
    fclose(f);
    PolarCode::ListResult r = code.decode_scl_llr_list(v, 6);
    for (long b = 0; b < r.B; ++b) {
        printf("%d %d\n", (int)r.n_active[b], (int)r.winner[b]);
        for (int l = 0; l < r.L; ++l) {
            unsigned long long bits;
            memcpy(&bits, &r.pm[b * r.L + l], 8);
            printf("%d %016llx ", (int)r.crc_ok[b * r.L + l], bits);
            for (int k = 0; k < r.K; ++k) putchar('0' + r.cand[((size_t)b * r.L + l) * r.K + k]);
            putchar('\n');
        }
    }
    return 0;
}
"""


def test_cpp_mirror(built_lib, oracle_built, tmp_path):
    from polar_amd import build
    o, g = _pair(6, 32, 8)
    B, L = 6, 6
    llr, _ = o.synth_llr(13, 0, B, o.snr_sqrt_linear(1.5))
    llr.tofile(str(tmp_path / "llr.bin"))
    (tmp_path / "main.cpp").write_text("#include <cstring>\n" + CPP_MAIN)
    exe = str(tmp_path / "list_main")
    here = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", build.INC, "-I", os.path.join(here, "cpp"), str(tmp_path / "main.cpp"),
                           "-o", exe, "-L", here, "-lpolar_amd", "-Wl,-rpath," + here,
                           "-Wl,-rpath," + (build._torch_lib() or "/opt/rocm/lib"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path / "llr.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    cand, pm, ok, na, win = g.decode_scl_llr_list(llr, L)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == B * (L + 1)
    for b in range(B):
        assert lines[b * (L + 1)].split() == [str(na[b]), str(win[b])]
        for l in range(L):
            f_ok, f_pm, f_bits = lines[b * (L + 1) + 1 + l].split()
            assert int(f_ok) == ok[b, l] and int(f_pm, 16) == int(pm[b, l:l + 1].view(np.uint64)[0])
            assert f_bits == "".join(str(int(v)) for v in cand[b, l])
