"""Error analysis of the list decoder on the device: the path metric of given words (polar_path_metric_batch[_dev]) against the numpy
forced pass and, bit for bit, against the list kernel's own metrics; the sweep counters of polar_mc_batch_list against the numpy
statement of tests/list_stats_numpy.py; list_stats and the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

import list_stats_numpy as LS
import scl_list_numpy as S

pytestmark = pytest.mark.gpu
REL = 1e-10          # tests/test_scl_list.py: libm against the kernel's table-driven exp / log1p


def _pair(n, K, crc, srand=1):
    import ctypes as C
    import polar_amd
    from oracle_lib import Oracle
    o = Oracle(n, K, 0.32, crc, srand=srand)
    C.CDLL(None).srand(C.c_uint(srand))
    g = polar_amd.PolarCode(n, K, 0.32, crc)
    return o, g


def _close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    inf = np.isposinf(b)
    fin = ~inf
    return bool((np.isposinf(a) == inf).all() and (np.abs(a[fin] - b[fin]) <= REL * np.maximum(1.0, np.abs(b[fin]))).all())


# ---- 1. the metric against the numpy forced pass ------------------------------------------------------------------------------
# (n, K, crc, rows, words per row): the three list cases on their 64 rows, a working shape, and a code whose N doubles do not fit LDS
METRIC_CASES = [(c[0], c[1], c[2], S.LIST_ROWS, 4) for c in S.LIST_CASES] + [(10, 512, 8, 32, 4), (15, 16384, 0, 2, 4)]
_metric_inputs = {}


def _metric_case(case):
    """(oracle, handle, code, llr [B, N], words [B, R, K]: the sent word and R - 1 random ones), once per case."""
    if case not in _metric_inputs:
        n, K, crc, B, R = case
        o, g = _pair(n, K, crc)
        llr, sent = o.synth_llr(S.LIST_SEED, 0, B, o.snr_sqrt_linear(S.LIST_EBNO))
        words = np.random.default_rng(n).integers(0, 2, (B, R, K)).astype(np.uint8)
        words[:, 0] = sent
        _metric_inputs[case] = (o, g, S.Code(o), llr, words)
    return _metric_inputs[case]


@pytest.mark.parametrize("scale", [1.0, 50.0, 1000.0])      # 50: the min-sum branch of the f-node; 1000: log(1 + e^x) overflows to +inf
@pytest.mark.parametrize("case", METRIC_CASES)
def test_metric_against_numpy(built_lib, oracle_built, case, scale):
    o, g, code, llr, words = _metric_case(case)
    x = llr * scale
    got = g.path_metric(x, words)
    assert got.shape == words.shape[:2]
    want = np.stack([S.forced_path_metric(code, x[b], S.word(code, words[b])) for b in range(len(x))])
    assert _close(got, want), np.abs(got - want).max()
    if scale == 1000.0:
        assert np.isposinf(want).any()
    one = g.path_metric(x, words[:, 0])                                  # [B, K]: one word per row
    assert one.shape == (len(x),) and one.tobytes() == got[:, 0].tobytes()


def test_metric_formats(built_lib, oracle_built):
    """Every element format gives the float64 call's bits on the widened values; the device-resident form gives the host form's."""
    import torch
    from llr16_util import to_bf16_patterns, widen_bf16
    o, g, code, llr, words = _metric_case(METRIC_CASES[1])
    f32, f16, b16 = llr.astype(np.float32), llr.astype(np.float16), to_bf16_patterns(llr)
    for fmt, rows, wide in ((None, f32, f32.astype(np.float64)), (None, f16, f16.astype(np.float64)), ("bf16", b16, widen_bf16(b16))):
        want = g.path_metric(wide, words)
        assert g.path_metric(rows, words, fmt=fmt).tobytes() == want.tobytes(), (fmt, rows.dtype)
        assert _close(want, np.stack([S.forced_path_metric(code, wide[b], S.word(code, words[b])) for b in range(len(wide))]))
    B, R = words.shape[:2]
    pm = torch.full((B, R), -1.0, dtype=torch.float64, device="cuda")
    d_llr, d_words = torch.tensor(f16.view(np.int16), device="cuda"), torch.tensor(words, device="cuda")
    g.path_metric_dev(d_llr.data_ptr(), "f16", d_words.data_ptr(), B, R, pm.data_ptr())
    torch.cuda.synchronize()
    assert pm.cpu().numpy().tobytes() == g.path_metric(f16, words).tobytes()


# ---- 2. the metric against the list kernel, bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("n,K,crc,L", [(5, 16, 0, 4), (5, 16, 0, 1), (5, 16, 0, 3), (6, 32, 8, 8), (9, 256, 0, 2), (10, 512, 8, 8),
                                       (11, 1024, 16, 32)])
def test_metric_equals_the_list_kernels_bit_for_bit(built_lib, oracle_built, n, K, crc, L):
    """The list's own words fed back (R = L): wherever a row passed the CRC — its check bits are then the CRC matrix's, the path the
    forced pass walks — the two metrics are the same 64 bits. Rows decided with other check bits are another path."""
    o, g = _pair(n, K, crc)
    B = 64
    llr, _ = o.synth_llr(S.LIST_SEED, 0, B, o.snr_sqrt_linear(S.LIST_EBNO))
    cand, pm, ok, na, win = g.decode_scl_llr_list(llr, L)
    forced = g.path_metric(llr, cand)
    assert forced.shape == (B, L)
    valid = (ok == 1) & (np.arange(L)[None, :] < na[:, None])
    # (something is compared in most rows. A row without a single CRC-passing path has nothing to compare; on the CPU the numpy list
    # decoder finds a passing path in 47 of these 64 rows at (6, 32, 8, 8), and the oracle decodes 62 and 64 of them correctly — a
    # passing winner — at (10, 512, 8, 8) and (11, 1024, 16, 32))
    assert valid.any(axis=1).sum() >= B // 2
    diff = valid & (forced.view(np.uint64) != pm.view(np.uint64))
    assert not diff.any(), (int(diff.sum()), forced[diff][:4], pm[diff][:4])
    if crc == 0:
        assert valid.sum() == na.sum()


# ---- 3. the sweep counters -----------------------------------------------------------------------------------------------------
def _mc_list(g, T, Ls, axis, enabled=None, t0=0, stride=1, constellation=0, seed=LS.STATS_SEED):
    stats = np.zeros((len(Ls), len(axis), 5), np.uint64)
    g.mc_batch_list(seed, t0, T, stride, axis, Ls, np.ones((len(Ls), len(axis)), np.uint8) if enabled is None else enabled, stats,
                    constellation)
    return stats


@pytest.mark.parametrize("case", LS.STATS_CASES)
def test_sweep_counters_equal_numpy(built_lib, oracle_built, case):
    n, K, crc, L = case
    want = LS.reference(case)[4]
    _, g = _pair(n, K, crc)
    T = LS.STATS_T
    got = _mc_list(g, T, [L], [LS.STATS_EBNO])[0, 0]
    print(case, "device", got.tolist(), "numpy", want.tolist())
    assert got.tolist() == want.tolist()
    assert got[LS.RUN] == T
    err, run = np.zeros((1, 1), np.uint64), np.zeros((1, 1), np.uint64)
    g.mc_batch(LS.STATS_SEED, 0, T, 1, [LS.STATS_EBNO], [L], np.ones((1, 1), np.uint8), err, run)
    assert got[LS.ERR] == err[0, 0] and run[0, 0] == T
    # chunks of 7 trials
    g.debug_set("list_chunk_cw", 7)
    try:
        assert _mc_list(g, T, [L], [LS.STATS_EBNO])[0, 0].tolist() == got.tolist()
    finally:
        g.debug_set("list_chunk_cw", 0)
    # even and odd trials
    halves = _mc_list(g, T // 2, [L], [LS.STATS_EBNO], t0=0, stride=2) + _mc_list(g, T // 2, [L], [LS.STATS_EBNO], t0=1, stride=2)
    assert halves[0, 0].tolist() == got.tolist()


def test_sweep_points_list_sizes_and_a_disabled_cell(built_lib, oracle_built):
    _, g = _pair(6, 32, 8)
    T, Ls, axis = 128, [2, 8], [1.0, 2.0]
    en = np.array([[1, 0], [1, 1]], np.uint8)
    stats = np.full((2, 2, 5), 5, np.uint64)                               # (the call ADDS)
    g.mc_batch_list(3, 0, T, 1, axis, Ls, en, stats)
    assert (stats[0, 1] == 5).all()
    for li in range(2):
        for ie in range(2):
            if en[li, ie]:
                assert (stats[li, ie] - 5).tolist() == _mc_list(g, T, [Ls[li]], [axis[ie]], seed=3)[0, 0].tolist(), (li, ie)
    assert stats[1, 0, LS.ERR] > stats[1, 1, LS.ERR]


def test_sweep_cells_with_different_chunks_and_geometries(built_lib, oracle_built):
    """One call whose list sizes take groups of 2, 8 and 32 lanes (with and without a prefix pass) in chunks of 7, 7, 7 and 2 trials:
    every buffer is sized once for the largest before the first launch, and every cell counts what a call of its own counts."""
    _, g = _pair(10, 512, 8)
    T, Ls, axis = 23, [2, 8, 32], [1.0, 2.0]
    en = np.array([[1, 1], [0, 1], [1, 1]], np.uint8)
    g.debug_set("list_chunk_cw", 7)
    try:
        stats = np.full((3, 2, 5), 5, np.uint64)                           # (the call ADDS)
        g.mc_batch_list(3, 0, T, 1, axis, Ls, en, stats)
        alone = {(li, ie): _mc_list(g, T, [Ls[li]], [axis[ie]], seed=3)[0, 0] for li in range(3) for ie in range(2) if en[li, ie]}
    finally:
        g.debug_set("list_chunk_cw", 0)
    assert (stats[1, 0] == 5).all()
    for (li, ie), want in alone.items():
        assert (stats[li, ie] - 5).tolist() == want.tolist(), (li, ie)
        assert want[LS.RUN] == T


# ---- 4. BICM ------------------------------------------------------------------------------------------------------------------
def test_sweep_bicm(built_lib, oracle_built):
    import polar_amd
    _, g = _pair(8, 128, 8)
    T, L, snr = 256, 4, 6.0
    s = _mc_list(g, T, [L], [snr], constellation=polar_amd.ASK4_GRAY, seed=4)[0, 0]
    err, run = np.zeros((1, 1), np.uint64), np.zeros((1, 1), np.uint64)
    g.mc_batch_bicm(polar_amd.ASK4_GRAY, 4, 0, T, 1, [snr], [L], np.ones((1, 1), np.uint8), err, run)
    print("bicm", s.tolist(), int(err[0, 0]))
    assert s[LS.RUN] == T and s[LS.ERR] == err[0, 0]
    assert s[LS.MISS] <= s[LS.ERR] and s[LS.ML] <= s[LS.UNDET] <= s[LS.ERR]
    assert (_mc_list(g, T, [L], [snr], constellation="ask4-gray", seed=4)[0, 0] == s).all()


# ---- 5. list_stats ------------------------------------------------------------------------------------------------------------
def test_list_stats_stops_and_rates(built_lib, oracle_built):
    _, g = _pair(5, 16, 0)
    r = g.list_stats([LS.STATS_EBNO], [4], max_runs=1000, max_err=20, seed=1, batch=64)
    st = r["stats"][0, 0]
    assert st[LS.ERR] > 20 and st[LS.RUN] % 64 == 0 and 64 <= st[LS.RUN] < 1000
    # ... and the round before had not reached max_err
    assert _mc_list(g, int(st[LS.RUN]) - 64, [4], [LS.STATS_EBNO])[0, 0, LS.ERR] <= 20
    assert _mc_list(g, int(st[LS.RUN]), [4], [LS.STATS_EBNO])[0, 0].tolist() == st.tolist()
    for name, col in (("bler", LS.ERR), ("miss_rate", LS.MISS), ("undetected_rate", LS.UNDET), ("ml_bound", LS.ML)):
        assert r[name].shape == (1, 1) and r[name][0, 0] == st[col] / st[LS.RUN]
    # max_runs is never exceeded, whatever the rounds; a point that reached max_err stops, the other goes on
    r2 = g.list_stats([0.0, 4.0], [1, 4], max_runs=200, max_err=30, seed=1, batch=64)
    run, err = r2["stats"][:, :, LS.RUN], r2["stats"][:, :, LS.ERR]
    assert (run <= 200).all() and run[1, 1] == 200 and err[1, 1] <= 30
    assert err[0, 0] > 30 and run[0, 0] < 200
    r3 = g.list_stats([LS.STATS_EBNO], [4], max_runs=100, max_err=1000, seed=1)
    assert r3["stats"][0, 0, LS.RUN] == 100


# ---- 6. the C++ mirror --------------------------------------------------------------------------------------------------------
CPP_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "PolarCode.hpp"
int main(int argc, char **argv) {
    // argv[1]: doubles, B rows of 64; argv[2]: bytes, B x 3 words of 32 bits. Prints the metrics' bits, then the counters of a sweep
    PolarCode code(6, 32, 0.32, 8);
    std::vector<double> v;
    std::vector<uint8_t> w;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    double x;
    while (fread(&x, sizeof x, 1, f) == 1) v.push_back(x);
    fclose(f);
    f = fopen(argv[2], "rb");
    if (!f) return 2;
    int c;
    while ((c = fgetc(f)) != EOF) w.push_back((uint8_t)c);
    fclose(f);
    for (double m : code.path_metric(v, w, 3)) {
        unsigned long long bits;
        memcpy(&bits, &m, 8);
        printf("%016llx\n", bits);
    }
    PolarCode::ListStats s = code.list_stats({1.0, 2.0}, {2, 8}, 300, 25, 7, 100);
    for (size_t i = 0; i < s.stats.size(); ++i) printf("%llu\n", (unsigned long long)s.stats[i]);
    for (size_t i = 0; i < s.bler.size(); ++i) printf("%.17g %.17g %.17g %.17g\n", s.bler[i], s.miss_rate[i], s.undetected_rate[i], s.ml_bound[i]);
    return 0;
}
"""


def test_cpp_mirror(built_lib, oracle_built, tmp_path):
    from polar_amd import build
    o, g = _pair(6, 32, 8)
    B, R = 6, 3
    llr, sent = o.synth_llr(13, 0, B, o.snr_sqrt_linear(1.5))
    words = np.random.default_rng(6).integers(0, 2, (B, R, 32)).astype(np.uint8)
    words[:, 0] = sent
    llr.tofile(str(tmp_path / "llr.bin"))
    words.tofile(str(tmp_path / "words.bin"))
    (tmp_path / "main.cpp").write_text(CPP_MAIN)
    exe = str(tmp_path / "stats_main")
    here = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", build.INC, "-I", os.path.join(here, "cpp"), str(tmp_path / "main.cpp"),
                           "-o", exe, "-L", here, "-lpolar_amd", "-Wl,-rpath," + here,
                           "-Wl,-rpath," + (build._torch_lib() or "/opt/rocm/lib"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path / "llr.bin"), str(tmp_path / "words.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    pm = g.path_metric(llr, words)
    assert [int(x, 16) for x in lines[:B * R]] == pm.view(np.uint64).reshape(-1).tolist()
    want = g.list_stats([1.0, 2.0], [2, 8], max_runs=300, max_err=25, seed=7, batch=100)
    assert [int(x) for x in lines[B * R:B * R + 20]] == want["stats"].reshape(-1).tolist()
    rates = np.array([[float(v) for v in l.split()] for l in lines[B * R + 20:]])
    assert rates.shape == (4, 4)
    for k, name in enumerate(("bler", "miss_rate", "undetected_rate", "ml_bound")):
        assert (rates[:, k] == want[name].reshape(-1)).all(), name
