"""GPU suite of the symbol-domain BICM receiver: the demapper kernel pinned to the oracle and to a host
evaluation of include/polar_synth.h, checked against the independent numpy formulas, and decoding from received symbols
against decode_scl_llr on the demapped LLRs — device pointers and host pointers, float64 and float32 symbols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import golden_util as G
import polarm_numpy as PM
from oracle_lib import Oracle
from test_bicm_rx import NAMES, SP_LEVELS, numpy_levels  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBITS = {1: 2, 2: 3, 3: 4, 4: 1, 5: 2, 6: 3, 7: 4}

HOST_DEMAP_C = r"""
#include "polar_synth.h"
/* rows of M symbols -> rows of N positions, the tail as synth_kernel leaves it */
void host_demap(int id, const double *y, long B, int M, int N, double n0, double *llr, double *p1) {
    const int nb = polar_const_nbits(id);
    const double norm = polar_const_norm(id);
    for (long b = 0; b < B; ++b) {
        for (int i = 0; i < M; ++i)
            polar_synth_bicm_demap2(id, norm, y[b * M + i], n0, llr + b * N + (long)i * nb, p1 + b * N + (long)i * nb);
        for (int i = M * nb; i < N; ++i) { llr[b * N + i] = 0.0; p1[b * N + i] = 0.5; }
    }
}
"""


def _sigma_n0(snr_db):
    s = np.sqrt(0.5) * 10 ** (-snr_db / 20)          # main_MC_CC_Comparison.m:90
    return s, s * s


def _bits(a):
    """bit patterns of doubles: == on these also tells NaNs and signed zeros apart"""
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def host_demap(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_demap")
    (d / "host_demap.c").write_text(HOST_DEMAP_C)
    so = str(d / "libhost_demap.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           str(d / "host_demap.c"), "-o", so])
    lib = C.CDLL(so)

    def run(cid, y, N, n0):
        y = np.ascontiguousarray(y, np.float64)
        B, M = y.shape
        llr, p1 = np.zeros((B, N)), np.zeros((B, N))
        dp = C.POINTER(C.c_double)
        lib.host_demap(C.c_int(cid), y.ctypes.data_as(dp), C.c_long(B), C.c_int(M), C.c_int(N), C.c_double(n0),
                       llr.ctypes.data_as(dp), p1.ctypes.data_as(dp))
        return llr, p1
    return run


def _cfg5():
    import polar_amd
    c, frozen, order, crcm = G.tables("cfg5_n10_k512_ask16")
    g = polar_amd.PolarCode.from_tables(10, 512, 0, frozen, order, None)
    o = Oracle(10, 512, 0.5, 0)
    o.set_tables(frozen, order)
    return g, o


def _code(n, K, crc):
    import polar_amd
    C.CDLL(None).srand(C.c_uint(1))
    return polar_amd.PolarCode(n, K, 0.32, crc)


def _synth(g, cid, seed, t0, B, snr):
    """(symbols [B][M], LLRs [B][N], info [B][K]) of the same trials, as device tensors"""
    import torch
    M = g.N // NBITS[cid]
    d_y = torch.empty((B, M), dtype=torch.float64, device="cuda")
    d_llr = torch.empty((B, g.N), dtype=torch.float64, device="cuda")
    d_info = torch.empty((B, g.K), dtype=torch.uint8, device="cuda")
    g.synth_bicm_sym_dev(cid, seed, t0, B, snr, d_y.data_ptr(), d_info.data_ptr())
    g.synth_bicm_llr_dev(cid, seed, t0, B, snr, d_llr.data_ptr())
    torch.cuda.synchronize()
    return d_y, d_llr, d_info


@pytest.mark.parametrize("cid", [1, 2, 3, 6])
def test_demapper_is_pinned_to_the_oracle_and_the_header(built_lib, oracle_built, host_demap, cid):
    """synth_bicm_sym_dev -> compute_llr_bicm on the device == synth_bicm_llr_dev of the same trials == the oracle (ids the
    oracle's front end knows), every double; p1 == a host evaluation of polar_synth_bicm_demap2 built from the header; the
    8-ASK tail is exactly 0.0 / 0.5."""
    import torch
    import polar_amd
    g, o = _cfg5()
    con = polar_amd.Constellation(cid)
    B, N = 70, 1024
    M = N // con.n_bits
    for snr in (6.0, 11.5):
        _, n0 = _sigma_n0(snr)
        d_y, d_llr, d_info = _synth(g, cid, 31, 1000, B, snr)
        got_llr = torch.full((B, N), 7.0, dtype=torch.float64, device="cuda")
        got_p1 = torch.full((B, N), 7.0, dtype=torch.float64, device="cuda")
        con.compute_llr_bicm_dev(d_y.data_ptr(), N, B, n0, got_llr.data_ptr(), got_p1.data_ptr())
        torch.cuda.synchronize()
        llr, p1, y = got_llr.cpu().numpy(), got_p1.cpu().numpy(), d_y.cpu().numpy()
        assert (_bits(llr) == _bits(d_llr.cpu().numpy())).all()
        if cid in (1, 2, 3):
            o_llr, o_info = o.synth_bicm_llr(cid, 31, 1000, B, snr)
            assert (llr == o_llr).all() and (_bits(llr) == _bits(o_llr)).all()
            assert (d_info.cpu().numpy() == o_info).all()
        h_llr, h_p1 = host_demap(cid, y, N, n0)
        assert (_bits(p1) == _bits(h_p1)).all() and (_bits(llr) == _bits(h_llr)).all()
        assert (llr[:, M * con.n_bits:] == 0.0).all() and (p1[:, M * con.n_bits:] == 0.5).all()
        assert (N - M * con.n_bits) == (1 if con.n_bits == 3 else 0)
        # either output alone, host pointers, float32 symbols
        only_p1 = torch.full((B, N), 7.0, dtype=torch.float64, device="cuda")
        con.compute_llr_bicm_dev(d_y.data_ptr(), N, B, n0, 0, only_p1.data_ptr())
        only_llr = torch.full((B, N), 7.0, dtype=torch.float64, device="cuda")
        con.compute_llr_bicm_dev(d_y.data_ptr(), N, B, n0, only_llr.data_ptr(), 0)
        torch.cuda.synchronize()
        assert (_bits(only_p1.cpu().numpy()) == _bits(p1)).all() and (_bits(only_llr.cpu().numpy()) == _bits(llr)).all()
        hp1, hllr = con.compute_llr_bicm(y, n0, N)
        assert (_bits(hp1) == _bits(p1)).all() and (_bits(hllr) == _bits(llr)).all()
        y32 = y.astype(np.float32)
        fp1, fllr = con.compute_llr_bicm(y32, n0, N)
        w_llr, w_p1 = host_demap(cid, y32.astype(np.float64), N, n0)
        assert (_bits(fp1) == _bits(w_p1)).all() and (_bits(fllr) == _bits(w_llr)).all()
        d_y32 = d_y.to(torch.float32)
        con.compute_llr_bicm_dev(d_y32.data_ptr(), N, B, n0, got_llr.data_ptr(), got_p1.data_ptr(), f32=True)
        torch.cuda.synchronize()
        assert (_bits(got_llr.cpu().numpy()) == _bits(w_llr)).all() and (_bits(got_p1.cpu().numpy()) == _bits(w_p1)).all()
        # rows that are not 16-byte aligned take the scalar stores: same doubles
        pad = torch.full((B * N + 1,), 7.0, dtype=torch.float64, device="cuda")
        con.compute_llr_bicm_dev(d_y.data_ptr(), N, B, n0, pad.data_ptr() + 8, 0)
        torch.cuda.synchronize()
        assert (_bits(pad[1:].cpu().numpy().reshape(B, N)) == _bits(llr)).all() and float(pad[0]) == 7.0


# |llr| bound of the formula check. polar_synth_exp_neg flushes e^x to zero for x < -708 where libm goes on into the denormals;
# the two can only disagree beyond rounding where a flushed term DOMINATES one of the two sums of a level. The nearest point's
# exponent is at least -36 for a symbol inside the constellation or within 8.5 sigma of its ends (Box-Muller on 52-bit uniforms
# gives |z| <= sqrt(2 * 52 ln 2) = 8.5), so with |llr| = |e0 - e1| < 600 the smaller dominant exponent is above -636: 72 above
# the flush, and every flushed term is below e^-72 of the sum it is missing from.
LLR_BOUND = 600.0


@pytest.mark.parametrize("name", sorted(NAMES))
def test_demapper_against_the_independent_numpy_formulas(built_lib, numpy_levels, name):
    """Device LLR and p1 against polarm_numpy.compute_llr_bicm (libm exp / log, numpy sums) on the same y, at the tolerance
    tests/test_bicm.py grants libm against the fixed-order routines, over the entries with |llr| < LLR_BOUND; the share of
    entries left out is at most 1 % (SNRs of 5 and 13 dB: the numpy side alone decides it)."""
    import polar_amd
    cid = NAMES[name]
    con = polar_amd.Constellation(name)
    pts, nb = numpy_levels.constellation(cid)
    rng = np.random.default_rng(100 + cid)
    B, N = 64, 1024
    M = N // nb
    for snr in (5.0, 13.0):
        sigma, n0 = _sigma_n0(snr)
        y = pts[rng.integers(0, len(pts), (B, M))] + sigma * rng.standard_normal((B, M))
        want_p1, want_llr = numpy_levels.compute_llr_bicm(y.reshape(-1), n0, cid)
        p1, llr = con.compute_llr_bicm(y, n0, N)
        p1, llr = p1[:, : M * nb].reshape(-1), llr[:, : M * nb].reshape(-1)
        keep = np.abs(want_llr) < LLR_BOUND
        left_out = 1.0 - keep.mean()
        print(f"{name} snr {snr}: |llr| < {LLR_BOUND}: {100 * left_out:.4f} % of {keep.size} entries left out, "
              f"max |llr| {np.abs(want_llr).max():.1f}")
        assert left_out <= 0.01
        assert np.allclose(llr[keep], want_llr[keep], rtol=1e-9, atol=1e-9)
        assert np.allclose(p1[keep], want_p1[keep], rtol=1e-9, atol=1e-9)


def _u64(t):
    import torch
    return t.view(torch.int64)


@pytest.mark.parametrize("cfg", ["ask16-gray-n10", "ask4-gray-n11", "ask8-gray-n10"])
@pytest.mark.parametrize("crc", [0, 16])
def test_decode_from_symbols_equals_decode_from_llrs_on_device(built_lib, oracle_built, cfg, crc):
    """decode_bicm_dev(y): decoded bits and path metrics bit for bit those of decode_scl_llr_dev on the synthesised LLRs of the
    same trials, L in {1, 2, 4, 8, 32}, batch kernels and one-codeword-per-wave kernels; configuration 5 at L = 1 and 8 also
    against the oracle's decode of the oracle's own LLRs."""
    import torch
    cid, n, snr = {"ask16-gray-n10": (3, 10, 12.0), "ask4-gray-n11": (1, 11, 4.0), "ask8-gray-n10": (2, 10, 8.0)}[cfg]
    o = None
    if cfg == "ask16-gray-n10" and crc == 0:
        g, o = _cfg5()
    else:
        g = _code(n, 1 << (n - 1), crc)
    B = 200
    _, n0 = _sigma_n0(snr)
    d_y, d_llr, _ = _synth(g, cid, 5, 40, B, snr)
    d_y32 = d_y.to(torch.float32)
    for L in (1, 2, 4, 8, 32):
        for lat in (0, -1):                      # default dispatch (latency kernels where they apply), then the batch kernels
            g.debug_set("lat_max_b", lat)
            want = torch.zeros((B, g.K), dtype=torch.uint8, device="cuda")
            got = torch.ones((B, g.K), dtype=torch.uint8, device="cuda")
            want_pm = torch.zeros(B, dtype=torch.float64, device="cuda")
            got_pm = torch.ones(B, dtype=torch.float64, device="cuda")
            g.decode_scl_llr_dev(d_llr.data_ptr(), B, L, want.data_ptr(), want_pm.data_ptr())
            g.decode_bicm_dev(cid, d_y.data_ptr(), n0, B, L, got.data_ptr(), got_pm.data_ptr())
            torch.cuda.synchronize()
            assert torch.equal(got, want), (cfg, crc, L, lat)
            assert torch.equal(_u64(got_pm), _u64(want_pm)), (cfg, crc, L, lat)
            if L == 1:                           # without a metric list size 1 takes the pruned SC kernel
                got.fill_(1)
                g.decode_scl_llr_dev(d_llr.data_ptr(), B, L, want.data_ptr())
                g.decode_bicm_dev(cid, d_y.data_ptr(), n0, B, L, got.data_ptr())
                torch.cuda.synchronize()
                assert torch.equal(got, want), (cfg, crc, L, lat)
            if o is not None and L in (1, 8) and lat == 0:
                o_llr, _ = o.synth_bicm_llr(cid, 5, 40, B, snr)
                assert (got.cpu().numpy() == o.decode_scl_llr(o_llr, L)).all(), (L,)
        g.debug_set("lat_max_b", 0)
    # float32 symbols: the LLRs of the widened floats
    import polar_amd
    con = polar_amd.Constellation(cid)
    llr32 = torch.empty((B, g.N), dtype=torch.float64, device="cuda")
    con.compute_llr_bicm_dev(d_y32.data_ptr(), g.N, B, n0, llr32.data_ptr(), f32=True)
    for L in (1, 8):
        want = torch.zeros((B, g.K), dtype=torch.uint8, device="cuda")
        got = torch.ones((B, g.K), dtype=torch.uint8, device="cuda")
        g.decode_scl_llr_dev(llr32.data_ptr(), B, L, want.data_ptr())
        g.decode_bicm_dev(cid, d_y32.data_ptr(), n0, B, L, got.data_ptr(), f32=True)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (cfg, crc, L, "f32")


def test_decode_from_symbols_host_pointers(built_lib):
    """decode_bicm == decode_scl_llr(compute_llr_bicm(y)) for float64 and float32 symbols: B in {1, 7, 300, 5000} and a batch
    the dispatch rule pipelines. The rule is applied to the LLR bytes the symbols stand for: list size 1 pipelines from 32 MiB
    (4096 rows of N = 1024) when the batch exceeds a chunk, list size 8 from one round of resident waves
    (CUs * 16 * 8 codewords); below that one copy in, one decode, one copy out."""
    import torch
    import polar_amd
    g, _ = _cfg5()
    con = polar_amd.Constellation("ask16-gray")
    snr = 12.0
    _, n0 = _sigma_n0(snr)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = {1: 6000, 8: cus * 16 * 8}
    Bmax = max(big.values())
    d_y, _, _ = _synth(g, 3, 9, 0, Bmax, snr)
    y = d_y.cpu().numpy()
    y32 = y.astype(np.float32)
    llr = con.compute_llr_bicm(y, n0, g.N)[1]
    llr32 = con.compute_llr_bicm(y32.astype(np.float64), n0, g.N)[1]
    for L in (1, 8):
        want = g.decode_scl_llr(llr, L)
        assert g.debug_get("host_chunks") >= 2           # (the LLR path pipelines the largest batch ...)
        want32 = g.decode_scl_llr(llr32, L)
        for B in (1, 7, 300, 5000, big[L]):
            piped = B == big[L] or (L == 1 and B == 5000)
            got = g.decode_bicm(y[:B], n0, "ask16-gray", L)
            chunks = g.debug_get("host_chunks")
            assert (got == want[:B]).all(), (L, B)
            assert (chunks >= 2) if piped else (chunks == 0), (L, B, chunks)          # (... and so does the symbol path)
            got = g.decode_bicm(y32[:B], n0, con, L)
            assert (got == want32[:B]).all(), (L, B, "f32")
            assert (g.debug_get("host_chunks") >= 2) if piped else (g.debug_get("host_chunks") == 0), (L, B, "f32")
        # the same dispatch as the LLR path for the same B
        g.decode_scl_llr(llr[:5000], L)
        c_llr = (g.debug_get("host_chunks"), g.debug_get("host_chunk_cw"), g.debug_get("host_lanes"))
        g.decode_bicm(y[:5000], n0, "ask16-gray", L)
        assert c_llr == (g.debug_get("host_chunks"), g.debug_get("host_chunk_cw"), g.debug_get("host_lanes"))
    # one codeword, [M] in -> [K] out; a caller's output array
    assert (g.decode_bicm(y[3], n0, "ask16-gray", 4) == g.decode_scl_llr(llr[3], 4)).all()
    out = np.zeros((7, g.K), np.uint8)
    assert g.decode_bicm(y[:7], n0, "ask16-gray", 2, out=out) is out and (out == g.decode_scl_llr(llr[:7], 2)).all()


def test_modulate_and_points(built_lib, numpy_levels):
    """Constellation.modulate(encode(info)) against polarm_numpy.modulate for all ids: the symbol indices exactly, the values
    as exactly as the points agree (1 ulp: numpy's mean sums pairwise)."""
    import polar_amd
    g = _code(10, 512, 0)
    info = np.random.default_rng(3).integers(0, 2, (4, 512)).astype(np.uint8)
    coded = g.encode(info)
    for name, cid in NAMES.items():
        con = polar_amd.Constellation(name)
        pts, nb = numpy_levels.constellation(cid)
        assert (np.abs(con.points - pts) <= np.spacing(np.abs(pts))).all()
        got = con.modulate(coded)
        for b in range(4):
            want, sym = numpy_levels.modulate(coded[b], cid)
            assert (got[b] == con.points[sym]).all()
            assert (np.abs(got[b] - want) <= np.spacing(np.abs(want))).all()
            if (con.points == pts).all():
                assert (got[b] == want).all()


def test_refusals_leave_the_handle_usable(built_lib):
    import torch
    import polar_amd
    g, _ = _cfg5()
    _, n0 = _sigma_n0(12.0)
    B = 20
    d_y, d_llr, _ = _synth(g, 3, 2, 0, B, 12.0)
    y = d_y.cpu().numpy()
    d_out = torch.zeros((B, g.K), dtype=torch.uint8, device="cuda")
    ok = dict(c=3, y=d_y.data_ptr(), n0=n0, B=B, L=4, out=d_out.data_ptr())
    for bad in (dict(c=0), dict(c=8), dict(c=0x103), dict(y=0), dict(out=0), dict(n0=0.0), dict(n0=-1.0), dict(n0=float("nan")),
                dict(n0=float("inf")), dict(L=0), dict(L=65), dict(B=-1)):
        a = dict(ok, **bad)
        with pytest.raises(polar_amd.PolarError):
            g.decode_bicm_dev(a["c"], a["y"], a["n0"], a["B"], a["L"], a["out"])
        with pytest.raises(polar_amd.PolarError):
            g.decode_bicm_dev(a["c"], a["y"], a["n0"], a["B"], a["L"], a["out"], f32=True)
    g.decode_bicm_dev(3, d_y.data_ptr(), n0, 0, 4, d_out.data_ptr())                 # B = 0
    con = polar_amd.Constellation(3)
    d_l = torch.zeros((B, g.N), dtype=torch.float64, device="cuda")
    for bad in (dict(y=0), dict(n0=0.0), dict(n0=float("nan")), dict(B=-1), dict(N=0), dict(llr=0)):
        a = dict(dict(y=d_y.data_ptr(), N=g.N, B=B, n0=n0, llr=d_l.data_ptr()), **bad)
        with pytest.raises(polar_amd.PolarError):
            con.compute_llr_bicm_dev(a["y"], a["N"], a["B"], a["n0"], a["llr"], 0)
    for bad in (dict(c=0), dict(c=4), dict(c=9), dict(y=0), dict(B=-1)):             # (the BICM sweep has no BPSK: as synth_bicm_llr_dev)
        a = dict(dict(c=3, y=d_y.data_ptr(), B=B), **bad)
        with pytest.raises(polar_amd.PolarError):
            g.synth_bicm_sym_dev(a["c"], 2, 0, a["B"], 12.0, a["y"])
    for kw in (dict(n0=0.0), dict(c=0), dict(L=0), dict(L=65)):
        with pytest.raises(polar_amd.PolarError):
            g.decode_bicm(y, kw.get("n0", n0), kw.get("c", 3), kw.get("L", 4))
    with pytest.raises(polar_amd.PolarError, match="decode_bicm"):
        g.decode_bicm(np.zeros((B, g.N)), n0, 3, 4)
    # a valid call on the same handle after all of these
    want = torch.zeros((B, g.K), dtype=torch.uint8, device="cuda")
    g.decode_scl_llr_dev(d_llr.data_ptr(), B, 4, want.data_ptr())
    g.decode_bicm_dev(3, d_y.data_ptr(), n0, B, 4, d_out.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(d_out, want)
    assert (g.decode_bicm(y, n0, 3, 4) == want.cpu().numpy()).all()


def test_degenerate_row_far_outside_the_constellation(built_lib, host_demap):
    """One row far outside the constellation at a small n0: every exponential flushes to zero, p0 = p1 = 0, so p1 = 0 / 0 is NaN.
    The LLR of such a position is NOT non-finite: polar_synth_log is integer work on the bit pattern and maps the NaN of 0 / 0
    to 1024 ln 2 + ln 1.5 = 710.19 (include/polar_synth.h defines it so, on host and device alike), which the test pins against
    the host evaluation. decode_bicm gives what decode_scl_llr gives on those LLRs, at list sizes 1 and 8. One case, run once."""
    import polar_amd
    g, _ = _cfg5()
    con = polar_amd.Constellation("ask16-gray")
    M = g.N // 4
    y = np.zeros((3, M))
    rng = np.random.default_rng(1)
    y[0] = con.points[rng.integers(0, 16, M)]
    y[1] = 1.0e3                                  # (1e3 - 1.6)^2 / 2 / 1e-3 >> 708
    y[2] = con.points[rng.integers(0, 16, M)]
    n0 = 1.0e-3
    p1, llr = con.compute_llr_bicm(y, n0, g.N)
    h_llr, _ = host_demap(3, y, g.N, n0)
    assert np.isnan(p1[1]).all() and np.isfinite(p1[0]).all() and np.isfinite(p1[2]).all()
    print("row 1: llr", llr[1, :4], "p1", p1[1, :4], "| row 0: min |llr|", np.abs(llr[0]).min())
    assert (_bits(llr) == _bits(h_llr)).all()
    assert (llr[1] > 710.0).all() and (llr[1] < 710.4).all()
    # (rows 0 and 2 sit on the points: the nearest point of the other label is one spacing away, (2 / sqrt(85))^2 / 2 / n0 = 23.5)
    assert np.isfinite(llr[0]).all() and (np.abs(llr[0]) > 20).all()
    for L in (1, 8):
        assert (g.decode_bicm(y, n0, con, L) == g.decode_scl_llr(llr, L)).all(), L


CPP_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "PolarCode.hpp"
int main(int argc, char **argv) {
    // argv[1]: file of doubles, B rows of 256 symbols; prints B lines of 512 bits, then the same from floats
    std::vector<double> y;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    double v;
    while (fread(&v, sizeof v, 1, f) == 1) y.push_back(v);
    fclose(f);
    const double n0 = atof(argv[2]);
    PolarCode code(10, 512, 0.32, 0);
    std::vector<uint8_t> out = code.decode_bicm(y, n0, "ask16-gray", 4);
    std::vector<float> yf(y.begin(), y.end());
    std::vector<uint8_t> outf = code.decode_bicm(yf, n0, "ask16-gray", 4);
    std::vector<double> one(y.begin(), y.begin() + 256);
    std::vector<uint8_t> o1 = code.decode_bicm(one, n0, "ask16-gray", 4);
    for (const std::vector<uint8_t> *o : {&out, &outf, &o1}) {
        for (size_t i = 0; i < o->size(); ++i) { putchar('0' + (*o)[i]); if (i % 512 == 511) putchar('\n'); }
    }
    try { code.decode_bicm(y, n0, "qam16", 4); return 3; } catch (const std::out_of_range &) {}
    try { code.decode_bicm(y, 0.0, "ask16-gray", 4); return 4; } catch (const std::runtime_error &) {}
    return 0;
}
"""


def test_cpp_mirror_decodes_from_symbols(built_lib, tmp_path):
    """A program written against polar_amd/cpp/PolarCode.hpp decodes a batch from symbols: the bits of the Python layer."""
    import torch
    import polar_amd
    from polar_amd import build
    g = _code(10, 512, 0)
    B = 12
    _, n0 = _sigma_n0(12.0)
    d_y, _, _ = _synth(g, 3, 4, 0, B, 12.0)
    y = d_y.cpu().numpy()
    y.tofile(str(tmp_path / "y.bin"))
    (tmp_path / "main.cpp").write_text(CPP_MAIN)
    exe = str(tmp_path / "bicm_main")
    here = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", build.INC, "-I", os.path.join(here, "cpp"), str(tmp_path / "main.cpp"),
                           "-o", exe, "-L", here, "-lpolar_amd", "-Wl,-rpath," + here,
                           "-Wl,-rpath," + (build._torch_lib() or "/opt/rocm/lib"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path / "y.bin"), repr(float(n0))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = np.array([[int(ch) for ch in line] for line in r.stdout.strip().splitlines()], np.uint8)
    assert rows.shape == (2 * B + 1, 512)
    assert (rows[:B] == g.decode_bicm(y, n0, "ask16-gray", 4)).all()
    assert (rows[B:2 * B] == g.decode_bicm(y.astype(np.float32), n0, "ask16-gray", 4)).all()
    assert (rows[2 * B] == rows[0]).all()
