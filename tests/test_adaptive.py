"""Adaptive list decoding, the part that needs no GPU: the numpy model the device is compared against (tests/adaptive_numpy.py)
meets the conditions its shared inputs were chosen for, a single-stage schedule restates the oracle, and the three entry points
check their arguments before they touch a device."""
import ctypes as C

import numpy as np
import pytest

import adaptive_numpy as A

E_ARG, OK = -1, 0


@pytest.mark.parametrize("key,Ls,counts,errors,accepted", A.TABLE)
def test_shared_inputs_meet_their_conditions(oracle_built, key, Ls, counts, errors, accepted):
    """No TieError at any stage (adaptive() would raise), every stage non-empty, and the counts of the table: no GPU test can
    skip a row."""
    o, code, llr, sent, (info, pm, stage, ok) = A.reference(key, Ls)
    assert len(llr) == 256
    got = [int((stage == s).sum()) for s in range(len(Ls))]
    assert got == counts and min(got) > 0
    assert int((info != sent).any(axis=1).sum()) == errors
    assert int(ok.sum()) == accepted
    # crc_ok = 0 only at the last stage; an accepted word's stage is the first whose oracle decode it equals by construction
    assert (stage[ok == 0] == len(Ls) - 1).all()
    for s, L in enumerate(Ls):
        rows = np.nonzero(stage == s)[0]
        assert (o.decode_scl_llr(llr[rows], L) == info[rows]).all(), (s, L)
    c = A.counters(info, stage, ok, sent, len(Ls))
    assert c[A.RUN] == 256 and c[A.ERR] == errors and c[A.UNDET] <= c[A.ERR] and c[A.STAGE0:].sum() == 256


@pytest.mark.parametrize("key,L", A.SINGLE)
def test_single_stage_schedule_is_the_plain_decode(oracle_built, key, L):
    o, code, llr, sent, (info, pm, stage, ok) = A.reference(key, (L,))
    assert (info == o.decode_scl_llr(llr, L)).all()
    assert (stage == 0).all() and 0 < ok.sum() < 256


def test_abi_symbols_and_argument_checks(built_lib):
    import polar_amd
    L = polar_amd.lib()
    for name in ("polar_decode_scl_llr_adaptive_batch_dev", "polar_decode_scl_llr_adaptive_batch", "polar_mc_batch_adaptive"):
        assert hasattr(L, name), name
    assert L.polar_version() >= 200
    g = polar_amd.PolarCode(6, 32, 0.32, 8)
    g0 = polar_amd.PolarCode(6, 32, 0.32, 0)
    h = g._h
    buf = np.zeros(4096, np.uint8)
    p = C.c_void_p(buf.ctypes.data)            # (never dereferenced: every call below is refused or has B = 0 / T = 0)
    odd = C.c_void_p(buf.ctypes.data + 1)
    nul = C.c_void_p(0)

    def sched(Ls):
        a = np.array(Ls, np.uint8)
        return a, C.c_void_p(a.ctypes.data)

    def dev(h=h, llr=p, fmt=0, B=1, Ls=(1, 4, 32), n_s=None, out=p, no_sched=False):
        a, ap = sched(Ls)
        return L.polar_decode_scl_llr_adaptive_batch_dev(h, llr, C.c_int(fmt), C.c_long(B), nul if no_sched else ap,
                                                         C.c_int(len(Ls) if n_s is None else n_s), out, nul, nul, nul, nul)

    def host(h=h, llr=p, fmt=0, B=1, Ls=(1, 4, 32), n_s=None, out=p, no_sched=False):
        a, ap = sched(Ls)
        return L.polar_decode_scl_llr_adaptive_batch(h, llr, C.c_int(fmt), C.c_long(B), nul if no_sched else ap,
                                                     C.c_int(len(Ls) if n_s is None else n_s), out, nul, nul, nul)

    for f in (dev, host):
        assert f(h=nul) == E_ARG and f(llr=nul) == E_ARG and f(out=nul) == E_ARG and f(no_sched=True) == E_ARG
        assert f(n_s=0) == E_ARG and f(n_s=-1) == E_ARG and f(Ls=tuple(range(1, 10))) == E_ARG
        assert f(Ls=(0, 4)) == E_ARG and f(Ls=(4, 65)) == E_ARG and f(Ls=(65,)) == E_ARG
        assert f(Ls=(4, 4)) == E_ARG and f(Ls=(1, 8, 4)) == E_ARG and f(Ls=(2, 1)) == E_ARG
        assert f(fmt=-1) == E_ARG and f(fmt=4) == E_ARG
        assert f(llr=odd, fmt=2) == E_ARG and f(llr=odd, fmt=3) == E_ARG
        assert f(B=-1) == E_ARG
        assert f(h=g0._h) == E_ARG and f(h=g0._h, B=0) == E_ARG            # no CRC: nothing to accept on
        assert f(B=0) == OK and f(B=0, Ls=(3,)) == OK and f(B=0, fmt=3, Ls=tuple(range(1, 9))) == OK and f(B=0, Ls=(63, 64)) == OK
    assert dev(Ls=(4, 4)) == E_ARG and b"increasing" in L.polar_last_error()

    axis = np.array([1.5, 2.0])
    en = np.ones(2, np.uint8)
    stats = np.zeros((2, 3 + 8), np.uint64)

    def mc(h=h, const=0, T=1, stride=1, ax=C.c_void_p(axis.ctypes.data), n_e=2, Ls=(1, 4), n_s=None, no_sched=False,
           en=C.c_void_p(en.ctypes.data), st=C.c_void_p(stats.ctypes.data)):
        a, ap = sched(Ls)
        return L.polar_mc_batch_adaptive(h, C.c_int(const), C.c_uint64(1), C.c_uint64(0), C.c_long(T), C.c_long(stride), ax,
                                         C.c_int(n_e), nul if no_sched else ap, C.c_int(len(Ls) if n_s is None else n_s), en, st)

    assert mc(h=nul) == E_ARG and mc(ax=nul) == E_ARG and mc(no_sched=True) == E_ARG and mc(en=nul) == E_ARG and mc(st=nul) == E_ARG
    assert mc(const=polar_amd.RX_MLC | polar_amd.ASK4_SP) == E_ARG and mc(const=99) == E_ARG
    assert mc(T=-1) == E_ARG and mc(stride=0) == E_ARG and mc(n_e=0) == E_ARG
    assert mc(n_s=0) == E_ARG and mc(Ls=tuple(range(1, 10))) == E_ARG
    assert mc(Ls=(0,)) == E_ARG and mc(Ls=(65,)) == E_ARG and mc(Ls=(4, 4)) == E_ARG and mc(Ls=(8, 4)) == E_ARG
    assert mc(h=g0._h) == E_ARG
    assert mc(T=0) == OK and mc(T=0, const=polar_amd.ASK4_GRAY, Ls=(3, 6)) == OK
    assert (stats == 0).all()

    # the Python mirror refuses what the conversion to uint8 would wrap, and passes the rest on to the library
    for bad in ((1, 300), (-1, 4), (4, 4), (), (0,)):
        with pytest.raises(polar_amd.PolarError):
            g.decode_scl_llr_adaptive(np.zeros((1, 64)), bad)
    with pytest.raises(polar_amd.PolarError):
        g0.decode_scl_llr_adaptive(np.zeros((1, 64)), (1, 4))
    with pytest.raises(polar_amd.PolarError):
        g.decode_scl_llr_adaptive(np.zeros((2, 64), np.float32), (1, 4), fmt="bf16")
    with pytest.raises(polar_amd.PolarError):
        g.mc_batch_adaptive(1, 0, 0, 1, axis, (1, 4), en, np.zeros((2, 4), np.uint64))       # stats of the wrong shape
