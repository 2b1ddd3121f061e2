"""CPU suite of rate matching: the host entry points that need no device (polar_rm_pattern, polar_rm_forced,
polar_set_rate_match / polar_get_rate_match) against the plain numpy restatement of tests/rm_numpy.py, and that restatement's
design under the CPU oracle: encoded words are 0 at the known positions, clean rate-matched rows decode to the sent word."""
import warnings

import numpy as np
import pytest

import ga_numpy as G
import polar_amd
import rm_numpy as M
from oracle_lib import Oracle

PHI_DX = 1e-4
# (n, E per scheme): E < N for puncture / shorten, E >= N for repeat, both sides and both branches (Kp) for NR
CASES = [(n, sch, E, Kp) for n in (5, 7, 10) for sch, E, Kp in (
    ("puncture", (1 << n) * 3 // 4, None), ("puncture", 1, None), ("puncture", (1 << n) - 1, None),
    ("shorten", (1 << n) * 3 // 4, None), ("shorten", 1, None), ("shorten", (1 << n) - 1, None),
    ("repeat", 1 << n, None), ("repeat", (1 << n) + 1, None), ("repeat", (1 << n) * 5 // 4, None), ("repeat", 8 << n, None),
    ("nr", (1 << n) * 3 // 4, (1 << n) * 5 // 16), ("nr", (1 << n) * 3 // 4, (1 << n) // 2), ("nr", (1 << n) * 3 // 2, (1 << n) // 2),
    ("nr", (1 << n) * 25 // 32, (1 << n) * 3 // 8))]
# (n, K, crc, E, scheme, design Eb/N0): the shapes of tests/test_gpu_rm.py up to n = 10
DESIGNS = [(5, 8, 8, 24, "puncture", 2.0), (5, 8, 8, 24, "shorten", 2.0), (5, 8, 8, 40, "repeat", 2.0), (5, 8, 8, 33, "repeat", 2.0),
           (7, 48, 8, 100, "puncture", 2.0), (7, 48, 8, 100, "shorten", 2.0), (7, 32, 8, 100, "nr", 2.0), (7, 40, 8, 100, "nr", 2.0),
           (7, 56, 8, 100, "nr", 2.0), (7, 56, 8, 150, "nr", 2.0), (7, 56, 8, 200, "repeat", 2.0),
           (10, 384, 16, 800, "puncture", 1.5), (10, 384, 16, 800, "shorten", 1.5)]


@pytest.fixture(scope="module")
def tables():
    return G.phi_fwd(), G.phi_inv(PHI_DX)


@pytest.mark.parametrize("n,scheme,E,Kp", CASES)
def test_patterns_and_forced_leaves_equal_the_mirror(built_lib, n, scheme, E, Kp):
    sel, known = polar_amd.rate_match_pattern(n, E, scheme, Kp)
    wsel, wknown = M.pattern(n, E, scheme, Kp)
    assert sel.dtype == np.uint16 and (sel == wsel).all() and (known == wknown).all()
    assert not known[sel].any()
    f = polar_amd.rate_match_forced(n, sel, known)
    assert (f == M.forced(n, sel, known)).all()
    assert int(f.sum()) == int(M.punctured(n, sel, known).sum()) + int(known.sum())
    if scheme == "nr":
        y = M.nr_y(n)
        assert sorted(y.tolist()) == list(range(1 << n))
        # both branches of the bit selection are among the cases
        assert bool(known.any()) == (E < (1 << n) and 16 * Kp > 7 * E)


def test_forced_leaves_of_random_patterns(built_lib):
    rng = np.random.default_rng(5)
    for _ in range(20):
        n = 7
        N = 1 << n
        perm = rng.permutation(N)
        n_known, n_sent = int(rng.integers(0, 20)), int(rng.integers(40, 100))
        known = np.zeros(N, np.uint8)
        known[perm[:n_known]] = 1
        sel = rng.choice(perm[n_known:n_known + n_sent], int(rng.integers(n_sent, 2 * n_sent)))
        f = polar_amd.rate_match_forced(n, sel, known)
        assert (f == M.forced(n, sel, known)).all()


def _code(n=5, K=8, crc=8, E=24, scheme="shorten"):
    g = polar_amd.PolarCode(n, K, 0.32, crc)
    sel, known = M.pattern(n, E, scheme, K + crc)
    return g, sel, known


def test_set_rate_match_round_trip_and_refusals(built_lib, tables):
    fwd, inv = tables
    d = M.design(5, 8, 8, 24, "shorten", 2.0, fwd, inv)
    cm = np.zeros((8, 8), np.uint8)
    g = polar_amd.PolarCode.from_tables(5, 8, 8, d["frozen"], d["order"], cm)
    assert g.rate_match_info() is None
    assert np.isnan(g.snr_sqrt_linear_rm(1.0))
    g.set_rate_match(d["sel"], d["known"], 512.0)
    sel, known, short = g.rate_match_info()
    assert (sel == d["sel"]).all() and (known == d["known"]).all() and short == 512.0
    assert g.snr_sqrt_linear_rm(1.5) == M.snr_sqrt_linear_rm(8, 24, 1.5)
    g.clear_rate_match()
    assert g.rate_match_info() is None
    N = 32
    # E out of range
    with pytest.raises(polar_amd.PolarError, match="E = 257"):
        g.set_rate_match(np.zeros(8 * N + 1, np.uint16))
    # sel[e] >= N: the first offender is named
    bad = d["sel"].copy(); bad[3] = N; bad[7] = N + 1
    with pytest.raises(polar_amd.PolarError, match=r"sel\[3\] = 32"):
        g.set_rate_match(bad, d["known"])
    # a known position that is also sent
    kn = d["known"].copy(); kn[5] = 1
    with pytest.raises(polar_amd.PolarError, match="position 5 is known and also sent"):
        g.set_rate_match(d["sel"], kn)
    # a forced leaf of a known position is unfrozen: a code that does not know about the shortening
    plain = polar_amd.PolarCode(5, 16, 0.32, 0)
    fz = plain.frozen_bits
    first = next((b, p) for p in np.nonzero(d["known"])[0] for b in range(N) if b & M.bitrev(int(p), 5) == M.bitrev(int(p), 5) and not fz[b])
    with pytest.raises(polar_amd.PolarError, match="leaf %d is unfrozen, but coded position %d is known" % first):
        plain.set_rate_match(d["sel"], d["known"])
    # short_llr
    for v in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(polar_amd.PolarError, match="short_llr"):
            g.set_rate_match(d["sel"], d["known"], v)
    assert g.rate_match_info() is None                      # nothing was set by a refused call
    # a punctured pattern whose zero-capacity leaves are unfrozen is accepted
    psel, pknown = M.pattern(5, 24, "puncture")
    full = polar_amd.PolarCode(5, 32, 0.32, 0)
    full.set_rate_match(psel, pknown)
    assert full.rate_match_info()[0].size == 24
    with pytest.raises(polar_amd.PolarError):
        polar_amd.rate_match_pattern(5, 32, "puncture")
    with pytest.raises(polar_amd.PolarError):
        polar_amd.rate_match_pattern(5, 31, "repeat")
    with pytest.raises(polar_amd.PolarError):
        polar_amd.rate_match_pattern(4, 12, "nr", 8)
    with pytest.raises(polar_amd.PolarError):
        polar_amd.rate_match_pattern(5, 8 * 32 + 1, "repeat")


def test_entry_points_need_a_pattern(built_lib):
    """POLAR_E_ARG before any device is touched (this test runs without one)."""
    g = polar_amd.PolarCode(5, 8, 0.32, 8)
    L = g._L
    import ctypes as C
    one = C.c_void_p(8)
    assert L.polar_rate_match_batch_dev(g._h, one, C.c_long(1), one, None) == -1
    assert b"no rate-matching pattern" in L.polar_last_error()
    assert L.polar_rate_recover_batch_dev(g._h, one, C.c_int(0), C.c_long(1), one, None) == -1
    assert L.polar_decode_scl_llr_rm_batch_dev(g._h, one, C.c_int(0), C.c_long(1), C.c_int(1), one, None, None) == -1
    assert L.polar_synth_rm_llr_dev(g._h, C.c_uint64(1), C.c_uint64(0), C.c_long(1), C.c_double(1.0), one, None, None) == -1
    stats = np.zeros(3, np.uint64)
    with pytest.raises(polar_amd.PolarError, match="no rate-matching pattern"):
        g.mc_batch_rm(1, 0, 4, 1, [1.0], [1], [1], stats)


@pytest.mark.parametrize("n,K,crc,E,scheme,ebno", DESIGNS)
def test_designs_under_the_oracle(built_lib, oracle_built, tables, n, K, crc, E, scheme, ebno):
    fwd, inv = tables
    d = M.design(n, K, crc, E, scheme, ebno, fwd, inv)
    N = 1 << n
    # the design carries no unfrozen zero-capacity leaf (nor any other forced one), and the library accepts it without a warning
    assert not ((d["frozen"] == 0) & (d["forced"] == 1)).any()
    assert int((d["frozen"] == 0).sum()) == K + crc
    cm = np.random.default_rng(1).integers(0, 2, (crc, K)).astype(np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        g = polar_amd.PolarCode.from_tables(n, K, crc, d["frozen"], d["order"], cm)
    assert g.weak_leaves == 0
    g.set_rate_match(d["sel"], d["known"])
    o = Oracle(n, K, 0.32, crc, srand=1)
    o.set_tables(d["frozen"], d["order"])
    o.set_crc_matrix(cm)
    info = np.random.default_rng(n + E).integers(0, 2, (6, K)).astype(np.uint8)
    coded = np.stack([o.encode(i) for i in info])
    assert not coded[:, d["known"] != 0].any()
    # clean rows: LLR -4 s^2 (bit 1) / +4 s^2 (bit 0) at every transmit position, with a shortened LLR of 1000 and of +inf
    tx = coded[:, d["sel"]]
    rx = 8.0 * (1.0 - 2.0 * tx)
    for short in (1000.0, np.inf):
        llr = M.recover(rx, d["sel"], d["known"], short)
        assert (llr[:, M.punctured(n, d["sel"], d["known"])] == 0).all() and llr.shape == (6, N)
        for L in (1, 8):
            assert (o.decode_scl_llr(llr, L) == info).all()
