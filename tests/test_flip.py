"""SC-Flip, the part that needs no GPU: the numpy model the device is compared against (tests/flip_numpy.py) gives the counts its
shared inputs were chosen for and meets its margin conditions on every row, its first pass restates the oracle's list-of-1 decode,
the stored fixtures are what the model computes, and the three entry points check their arguments before they touch a device."""
import ctypes as C

import numpy as np
import pytest

import flip_numpy as F
import scl_list_numpy as S

E_ARG, E_UNSUPPORTED, OK = -1, -4, 0


def _consistent(code, llr, sent, r, T):
    """What every decode() result satisfies, whatever the inputs."""
    te = F.t_eff(code, T)
    ok, nd = r["crc_ok"] == 1, r["n_dec"].astype(int)
    info0 = S.split(code, r["u0"])[0]
    assert ((nd == 1) <= ok).all() and (nd[~ok] == te + 1).all() and (r["flip"][~ok] == -1).all() and (r["flip"][nd == 1] == -1).all()
    assert (r["info"][~ok] == info0[~ok]).all() and (r["info"][nd == 1] == info0[nd == 1]).all()
    retried = ok & (nd > 1)
    rows = np.flatnonzero(retried)
    assert (r["flip"][rows] == r["cand"][rows, nd[rows] - 2]).all()
    # a delivered retry is pass 0 up to the flipped leaf, inverted there
    for b in rows:
        u, _ = F.sc_pass(code, llr[b], [r["flip"][b]])
        c = int(r["flip"][b])
        assert (u[0, :c] == r["u0"][b, :c]).all() and u[0, c] == 1 - r["u0"][b, c] and not code.frozen[c]
        assert (S.split(code, u)[0][0] == r["info"][b]).all()
    # candidates: unfrozen, distinct, magnitudes ascending and those of pass 0's leaves
    for b in range(len(llr)):
        c = r["cand"][b, :te]
        assert (code.frozen[c] == 0).all() and len(set(c.tolist())) == te
        assert (np.diff(r["mag"][b, :te]) > 0).all() and (r["mag"][b, :te] == np.abs(r["leaf0"][b, c])).all()
        rest = np.setdiff1d(np.flatnonzero(code.frozen == 0), c)
        assert te == 0 or not len(rest) or np.abs(r["leaf0"][b, rest]).min() > r["mag"][b, te - 1]
    assert (r["cand"][:, te:] == -1).all() and np.isposinf(r["mag"][:, te:]).all()


@pytest.mark.parametrize("key,T,share,err,undet,dec", F.TABLE)
def test_table_rows(oracle_built, key, T, share, err, undet, dec):
    """No MarginError (decode() would raise), the counts and n_dec histograms of the table, pass 0 = the oracle's list of 1."""
    o, code, llr, sent, r = F.reference(key, T)
    assert len(llr) == 256
    gap, small = F.min_margins(code, r["leaf0"], T)
    print(key, T, F.shares(r), F.counters(r, sent).tolist(), "smallest gap %.3g, smallest |leaf| %.3g" % (gap, small))
    assert gap > 1e-6 and small > 1e-4                      # far from the 1e-9 the model refuses at
    assert F.shares(r) == share and sum(share) == 256
    c = F.counters(r, sent)
    assert c.tolist() == [256, err, undet, share[0], share[1], dec]
    assert np.bincount(r["n_dec"], minlength=T + 2).tolist() == F.TABLE_HIST[(key, T)]
    assert (S.split(code, r["u0"])[0] == o.decode_scl_llr(llr, 1)).all()
    _consistent(code, llr, sent, r, T)


def test_more_retries_only_help_the_failed_rows(oracle_built):
    """T = 4 against T = 8 on the same rows: a row T = 4 delivers is delivered the same way by T = 8."""
    _, code, llr, sent, r4 = F.reference((6, 32, 8), 4)
    r8 = F.reference((6, 32, 8), 8)[4]
    ok4 = r4["crc_ok"] == 1
    for k in ("info", "n_dec", "flip", "crc_ok"):
        assert (r4[k][ok4] == r8[k][ok4]).all(), k
    assert (r4["cand"] == r8["cand"][:, :4]).all() and (r4["mag"] == r8["mag"][:, :4]).all()
    r0 = F.decode(code, llr, 0)
    assert (r0["n_dec"] == 1).all() and (r0["crc_ok"] == (r4["n_dec"] == 1)).all() and r0["cand"].shape == (256, 0)
    assert (r0["info"][~ok4] == r4["info"][~ok4]).all()


@pytest.mark.parametrize("i", range(len(F.FIXTURES)))
def test_fixtures_are_the_model(oracle_built, i):
    """tests/golden/flip_fixtures.npz holds what the model computes from the oracle's channel, without a MarginError."""
    rows, key, T, seed, ebno, share = F.FIXTURES[i]
    o, code, llr, sent = F.fixture_inputs(i)
    r = F.decode(code, llr, T)
    fx = F.load_fixtures()[i]
    assert (fx["llr_sha"] == F.llr_sha(llr)).all() and (fx["sent"] == sent).all()
    for k in ("info", "crc_ok", "n_dec", "flip", "cand"):
        assert (fx[k] == r[k]).all() and fx[k].dtype == r[k].dtype, k
    assert fx["mag"].tobytes() == r["mag"].tobytes()
    print(key, T, ebno, F.shares(r), F.counters(r, sent).tolist(), F.min_margins(code, r["leaf0"], T))
    assert F.shares(r) == share and sum(share) == rows
    assert (S.split(code, r["u0"])[0] == o.decode_scl_llr(llr, 1)).all()
    if key == (5, 16, 8):
        c = F.counters(r, sent)
        assert F.t_eff(code, T) == 24 and c[F.ERR] == 28 and c[F.UNDET] == 5
        assert r["cand"].shape == (64, 64) and (r["cand"][:, 24:] == -1).all() and (r["n_dec"][r["crc_ok"] == 0] == 25).all()
        _consistent(code, llr, sent, r, T)


def test_clamp_and_all_zero_row(oracle_built):
    import list_stats_numpy as R
    code = S.Code(R.oracle(5, 16, 8))
    assert F.t_eff(code, 64) == 24 and F.t_eff(code, 24) == 24 and F.t_eff(code, 3) == 3 and F.t_eff(code, 0) == 0
    # the all-zero row: every leaf LLR is 0, every decision 0, the zero word passes; the candidates are the tie rule alone
    with pytest.raises(F.MarginError):
        F.decode(code, np.zeros((1, 32)), 5)
    r = F.decode(code, np.zeros((1, 32)), 5, check=False)
    assert (r["info"] == 0).all() and r["crc_ok"][0] == 1 and r["n_dec"][0] == 1 and r["flip"][0] == -1
    assert r["cand"][0].tolist() == np.flatnonzero(code.frozen == 0)[:5].tolist() and (r["mag"] == 0).all()
    # two equal magnitudes among the first T_eff + 1 are refused; the same pair further down is not looked at
    _, _, llr, _, r8 = F.reference((6, 32, 8), 8)
    code6 = S.Code(R.oracle(6, 32, 8))
    leaf = r8["leaf0"][:1].copy()
    c = r8["cand"][0]
    leaf[0, c[1]] = -abs(leaf[0, c[0]])
    with pytest.raises(F.MarginError):
        F.candidates(code6, leaf, 8)
    assert F.candidates(code6, leaf, 8, check=False)[0][0, :2].tolist() == sorted(c[:2].tolist())


def test_grid_edge_rows_meet_the_margins(oracle_built):
    """The rows of the grid edges of tests/test_gpu_flip.py raise no MarginError and behave as that test says: all first-pass at 8 dB,
    every retry spent and nothing delivered at -10 dB, every class present at 1.5 dB from 63 rows on; so do the rows above the
    kernel's grid cap and the rows of the min-sum test."""
    import list_stats_numpy as R
    o = R.oracle(6, 32, 8)
    code = S.Code(o)
    for B in F.EDGE_B:
        for ebno in F.EDGE_EBNO:
            llr, _ = o.synth_llr(F.edge_seed(B, ebno), 0, B, o.snr_sqrt_linear(ebno))
            r = F.decode(code, llr, F.EDGE_T)
            if ebno == 8.0:
                assert F.shares(r) == [B, 0, 0]
            elif ebno == -10.0:
                assert F.shares(r) == [0, 0, B] and (r["n_dec"] == F.EDGE_T + 1).all() and (r["flip"] == -1).all()
            elif B >= 63:
                assert min(F.shares(r)) > 0
    llr = F.reference((6, 32, 8), 8)[2]
    r = F.decode(code, F.MIN_SUM_SCALE * llr[:F.MIN_SUM_ROWS], 8)
    assert min(F.shares(r)) > 0
    B, seed, ebno, T = F.GRID_CAP_CASE
    llr, sent = o.synth_llr(seed, 0, B, o.snr_sqrt_linear(ebno))
    r = F.decode(S.Code(o), llr, T)
    assert min(F.shares(r)) > 0


def test_abi_symbols_and_argument_checks(built_lib):
    import polar_amd
    L = polar_amd.lib()
    for name in ("polar_decode_sc_flip_batch_dev", "polar_decode_sc_flip_batch", "polar_mc_batch_flip"):
        assert hasattr(L, name), name
    assert polar_amd.FL_N == 6 and polar_amd.FLIP_MAX == 64
    g = polar_amd.PolarCode(6, 32, 0.32, 8)
    g0 = polar_amd.PolarCode(6, 32, 0.32, 0)
    g13 = polar_amd.PolarCode(13, 4096, 0.32, 16)
    h = g._h
    buf = np.zeros(4096, np.uint8)
    p = C.c_void_p(buf.ctypes.data)            # (never dereferenced: every call below is refused or has B = 0 / T = 0)
    odd = C.c_void_p(buf.ctypes.data + 1)
    nul = C.c_void_p(0)

    def dev(h=h, llr=p, fmt=0, B=1, T=8, out=p):
        return L.polar_decode_sc_flip_batch_dev(h, llr, C.c_int(fmt), C.c_long(B), C.c_int(T), out, nul, nul, nul, nul, nul, nul)

    def host(h=h, llr=p, fmt=0, B=1, T=8, out=p):
        return L.polar_decode_sc_flip_batch(h, llr, C.c_int(fmt), C.c_long(B), C.c_int(T), out, nul, nul, nul, nul, nul)

    for f in (dev, host):
        assert f(h=nul) == E_ARG and f(llr=nul) == E_ARG and f(out=nul) == E_ARG
        assert f(T=-1) == E_ARG and f(T=65) == E_ARG
        assert f(fmt=-1) == E_ARG and f(fmt=4) == E_ARG
        assert f(llr=odd, fmt=2) == E_ARG and f(llr=odd, fmt=3) == E_ARG
        assert f(B=-1) == E_ARG
        assert f(h=g0._h) == E_ARG and f(h=g0._h, B=0) == E_ARG            # no CRC: nothing to accept on
        assert f(B=0) == OK and f(B=0, T=0) == OK and f(B=0, T=64, fmt=3) == OK
        assert f(h=g13._h) == E_UNSUPPORTED and f(h=g13._h, B=0) == E_UNSUPPORTED and f(h=g13._h, T=65) == E_ARG
    assert dev(T=65) == E_ARG and b"max_flips" in L.polar_last_error()

    axis = np.array([1.5, 2.0])
    en = np.ones(2, np.uint8)
    stats = np.zeros((2, 6), np.uint64)

    def mc(h=h, const=0, T=1, stride=1, ax=C.c_void_p(axis.ctypes.data), n_e=2, flips=8, en=C.c_void_p(en.ctypes.data),
           st=C.c_void_p(stats.ctypes.data)):
        return L.polar_mc_batch_flip(h, C.c_int(const), C.c_uint64(1), C.c_uint64(0), C.c_long(T), C.c_long(stride), ax, C.c_int(n_e),
                                     C.c_int(flips), en, st)

    assert mc(h=nul) == E_ARG and mc(ax=nul) == E_ARG and mc(en=nul) == E_ARG and mc(st=nul) == E_ARG
    assert mc(const=polar_amd.RX_MLC | polar_amd.ASK4_SP) == E_ARG and mc(const=99) == E_ARG
    assert mc(T=-1) == E_ARG and mc(stride=0) == E_ARG and mc(n_e=0) == E_ARG
    assert mc(flips=-1) == E_ARG and mc(flips=65) == E_ARG
    assert mc(h=g0._h) == E_ARG and mc(h=g13._h) == E_UNSUPPORTED
    assert mc(T=0) == OK and mc(T=0, const=polar_amd.ASK4_GRAY, flips=0) == OK
    assert (stats == 0).all()

    # the Python mirror passes its arguments on to the library
    for bad in (-1, 65):
        with pytest.raises(polar_amd.PolarError):
            g.decode_sc_flip(np.zeros((1, 64)), bad)
    with pytest.raises(polar_amd.PolarError):
        g0.decode_sc_flip(np.zeros((1, 64)), 4)
    with pytest.raises(polar_amd.PolarError):
        g.decode_sc_flip(np.zeros((2, 64), np.float32), 4, fmt="bf16")
    with pytest.raises(polar_amd.PolarError):
        g.mc_batch_flip(1, 0, 0, 1, axis, 4, en, np.zeros((2, 4), np.uint64))       # stats of the wrong shape
    with pytest.raises(polar_amd.PolarError):
        g.flip_stats(axis, 4, max_runs=0)
