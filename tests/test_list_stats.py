"""Error analysis of the list decoder, the part that needs no GPU: the numpy statement of the five counters
(tests/list_stats_numpy.py) on the inputs the GPU tests use — no tie, no metric gap an arithmetic difference could close, no
class the GPU tests rely on empty — and the argument checks of the three new entry points before they touch a device."""
import ctypes as C

import numpy as np
import pytest

import list_stats_numpy as LS


@pytest.mark.parametrize("case", LS.STATS_CASES)
def test_counters_of_the_shared_inputs(oracle_built, case):
    n, K, crc, L = case
    o, code, llr, sent, c, gap = LS.reference(case)          # (a TieError in any of the 256 rows raises here)
    print(case, "ERR MISS UNDET ML =", c[1:].tolist(), "smallest gap", gap)
    assert c[LS.RUN] == LS.STATS_T
    assert c[LS.ERR] == (o.decode_scl_llr(llr, L) != sent).any(axis=1).sum()
    assert c[LS.ML] <= c[LS.UNDET] <= c[LS.ERR] and c[LS.MISS] <= c[LS.ERR] < LS.STATS_T
    # a 1e-13 difference between two exp / log implementations cannot move the ML counter
    assert gap > 1e-6
    assert c[LS.ERR] > 0 and c[LS.MISS] > 0 and c[LS.UNDET] > 0
    if crc == 0:
        assert c[LS.UNDET] == c[LS.ERR]


def test_every_class_the_gpu_tests_rely_on_occurs(oracle_built):
    c = {case: LS.reference(case)[4] for case in LS.STATS_CASES}
    assert c[(6, 32, 8, 8)][LS.ERR] > c[(6, 32, 8, 8)][LS.MISS]                 # selection errors
    assert c[(6, 32, 8, 8)][LS.ML] > 0
    assert c[(7, 64, 8, 4)][LS.UNDET] > c[(7, 64, 8, 4)][LS.ML]                 # an undetected error that is not an ML error
    assert c[(5, 16, 0, 1)][LS.ERR] > c[(5, 16, 0, 1)][LS.ML] > 0
    assert c[(5, 16, 0, 4)][LS.ERR] > c[(5, 16, 0, 4)][LS.MISS]


E_ARG, OK = -1, 0


def test_abi_symbols_and_argument_checks(built_lib):
    import polar_amd
    L = polar_amd.lib()
    for name in ("polar_path_metric_batch_dev", "polar_path_metric_batch", "polar_mc_batch_list"):
        assert hasattr(L, name), name
    g = polar_amd.PolarCode(6, 32, 0.32, 8)
    h = g._h
    buf = np.zeros(4096, np.uint8)
    p = C.c_void_p(buf.ctypes.data)            # (never dereferenced: every call below is refused or has no rows)
    odd = C.c_void_p(buf.ctypes.data + 1)
    nul = C.c_void_p(0)

    def dev(h=h, llr=p, fmt=0, info=p, B=1, R=4, pm=p):
        return L.polar_path_metric_batch_dev(h, llr, C.c_int(fmt), info, C.c_long(B), C.c_int(R), pm, nul)

    def host(h=h, llr=p, fmt=0, info=p, B=1, R=4, pm=p):
        return L.polar_path_metric_batch(h, llr, C.c_int(fmt), info, C.c_long(B), C.c_int(R), pm)

    for f in (dev, host):
        assert f(h=nul) == E_ARG and f(llr=nul) == E_ARG and f(info=nul) == E_ARG and f(pm=nul) == E_ARG
        assert f(fmt=-1) == E_ARG and f(fmt=4) == E_ARG
        assert f(R=0) == E_ARG and f(R=65) == E_ARG
        assert f(B=-1) == E_ARG
        assert f(llr=odd, fmt=2) == E_ARG and f(llr=odd, fmt=3) == E_ARG
        assert f(B=0) == OK and f(B=0, R=64, fmt=3) == OK and f(B=0, R=1) == OK

    axis = np.array([1.5])
    Ls = np.array([4], np.uint8)
    en = np.ones(1, np.uint8)
    stats = np.full(5, 7, np.uint64)
    pa, pl, pe, ps = (C.c_void_p(a.ctypes.data) for a in (axis, Ls, en, stats))

    def mc(h=h, c=0, T=1, stride=1, axis=pa, n_e=1, Lp=pl, n_L=1, en=pe, st=ps):
        return L.polar_mc_batch_list(h, C.c_int(c), C.c_uint64(1), C.c_uint64(0), C.c_long(T), C.c_long(stride), axis, C.c_int(n_e),
                                     Lp, C.c_int(n_L), en, st)

    assert mc(h=nul) == E_ARG and mc(axis=nul) == E_ARG and mc(Lp=nul) == E_ARG and mc(en=nul) == E_ARG and mc(st=nul) == E_ARG
    assert mc(c=polar_amd.RX_MLC | polar_amd.ASK4_SP) == E_ARG and mc(c=polar_amd.RX_MLC) == E_ARG and mc(c=99) == E_ARG
    assert mc(T=-1) == E_ARG and mc(stride=0) == E_ARG and mc(n_e=0) == E_ARG and mc(n_L=0) == E_ARG
    for bad in (0, 65):
        Lb = np.array([bad], np.uint8)
        assert mc(Lp=C.c_void_p(Lb.ctypes.data)) == E_ARG
    assert mc(T=0) == OK and mc(T=0, c=polar_amd.ASK4_GRAY) == OK
    assert (stats == 7).all()
    with pytest.raises(polar_amd.PolarError):
        g.path_metric(np.zeros((2, 64)), np.zeros((3, 32), np.uint8))
    with pytest.raises(polar_amd.PolarError):
        g.path_metric(np.zeros((2, 64)), np.zeros((2, 65, 32), np.uint8))
    with pytest.raises(polar_amd.PolarError):
        g.mc_batch_list(1, 0, 1, 1, [1.5], [4], [1], np.zeros(4, np.uint64))
