"""List output of decode_scl_llr, the part that needs no GPU: the numpy list decoder the device is compared against
(tests/scl_list_numpy.py) restates the oracle, its forced pass restates its own list search, and the three new entry points
check their arguments before they touch a device."""
import ctypes as C

import numpy as np
import pytest

import scl_list_numpy as S

REL = 1e-10          # libm against another exp / log: the tolerance of test_winning_path_metric_matches_oracle


def _oracle(n, K, crc):
    from oracle_lib import Oracle
    return Oracle(n, K, 0.32, crc, srand=1)


def close(a, b):
    return abs(a - b) <= REL * max(1.0, abs(b))


@pytest.fixture(scope="module")
def survivors(oracle_built):
    """scl_list of all 3 x 64 rows — raises here if a tie makes any row undecidable: no row is skipped."""
    out = {}
    for case in S.LIST_CASES:
        n, K, crc, L = case
        o = _oracle(n, K, crc)
        code = S.Code(o)
        llr, _ = S.list_inputs(o)
        out[case] = (o, code, llr, [S.scl_list(code, llr[i], L) for i in range(S.LIST_ROWS)])
    return out


@pytest.mark.parametrize("case", S.LIST_CASES)
def test_numpy_list_decoder_restates_the_oracle(survivors, case):
    o, code, llr, rows = survivors[case]
    L = case[3]
    for i in range(S.LIST_ROWS):
        bits, pm = o.decode_scl_llr_pm(llr[i], L)
        b = S.best(rows[i])
        assert (b["info"] == bits).all(), i
        assert close(b["pm"], pm), (i, b["pm"], pm)
        assert len(rows[i]) == L and len({r["u"].tobytes() for r in rows[i]}) == L


def test_no_row_is_skipped_at_the_other_list_sizes(oracle_built):
    """The GPU tests also decode the first code at L = 1, 3 and 6: the seed keeps those tie-free as well."""
    n, K, crc, _ = S.LIST_CASES[0]
    o = _oracle(n, K, crc)
    code = S.Code(o)
    llr, _ = S.list_inputs(o)
    for L in (1, 3, 6):
        for i in range(S.LIST_ROWS):
            rows = S.scl_list(code, llr[i], L)
            assert len(rows) == L
            assert (S.best(rows)["info"] == o.decode_scl_llr(llr[i], L)).all()


@pytest.mark.parametrize("case", S.LIST_CASES)
def test_forced_path_metric_of_every_survivor(survivors, case):
    _, code, llr, rows = survivors[case]
    for i in range(S.LIST_ROWS):
        got = S.forced_path_metric(code, llr[i], np.stack([r["u"] for r in rows[i]]))
        for r, m in zip(rows[i], got):
            assert close(m, r["pm"]), (i, m, r["pm"])
            info, check = S.split(code, r["u"])
            assert (S.word(code, info, check) == r["u"]).all()
            assert bool(S.crc_ok(code, info, check)) == r["crc_ok"]


def test_forced_path_metric_works_at_2048(oracle_built):
    """The forced pass has no size limit: at N = 2048 (no CRC: the K bits are the whole decision vector) the path a list-size-1
    decode returns has the metric the oracle reports."""
    o = _oracle(11, 1024, 0)
    code = S.Code(o)
    llr, info = o.synth_llr(3, 0, 2, o.snr_sqrt_linear(1.5))
    for i in range(2):
        bits, pm = o.decode_scl_llr_pm(llr[i], 1)
        assert close(S.forced_path_metric(code, llr[i], S.word(code, bits)), pm)
    two = S.forced_path_metric(code, llr[0], np.stack([S.word(code, info[0]), S.word(code, 1 - info[0])]))
    assert two.shape == (2,) and two[0] < two[1]


# ---- ABI: the new symbols, and every argument error before the device -------------------------------------------------------
E_ARG, OK = -1, 0


def test_abi_symbols_and_argument_checks(built_lib):
    import polar_amd
    L = polar_amd.lib()
    for name in ("polar_decode_scl_llr_list_batch_dev", "polar_decode_scl_llr_list_batch", "polar_list_find_dev"):
        assert hasattr(L, name), name
    g = polar_amd.PolarCode(6, 32, 0.32, 8)
    h = g._h
    buf = np.zeros(4096, np.uint8)
    p = C.c_void_p(buf.ctypes.data)            # (never dereferenced: every call below is refused or has B = 0)
    odd = C.c_void_p(buf.ctypes.data + 1)
    nul = C.c_void_p(0)

    def dev(h=h, llr=p, fmt=0, B=1, Ls=4, cand=p):
        return L.polar_decode_scl_llr_list_batch_dev(h, llr, C.c_int(fmt), C.c_long(B), C.c_int(Ls), cand, nul, nul, nul, nul, nul)

    def host(h=h, llr=p, fmt=0, B=1, Ls=4, cand=p):
        return L.polar_decode_scl_llr_list_batch(h, llr, C.c_int(fmt), C.c_long(B), C.c_int(Ls), cand, nul, nul, nul, nul)

    for f in (dev, host):
        assert f(fmt=-1) == E_ARG and f(fmt=4) == E_ARG
        assert f(cand=nul) == E_ARG and f(llr=nul) == E_ARG and f(h=nul) == E_ARG
        assert f(Ls=0) == E_ARG and f(Ls=65) == E_ARG
        assert f(B=-1) == E_ARG
        assert f(llr=odd, fmt=2) == E_ARG and f(llr=odd, fmt=3) == E_ARG
        assert f(B=0) == OK and f(B=0, Ls=3) == OK and f(B=0, fmt=3, Ls=64) == OK

    def find(h=h, cand=p, na=p, info=p, B=1, Ls=4, rank=p):
        return L.polar_list_find_dev(h, cand, na, info, C.c_long(B), C.c_int(Ls), rank, nul)

    assert find(h=nul) == E_ARG and find(cand=nul) == E_ARG and find(na=nul) == E_ARG and find(info=nul) == E_ARG
    assert find(rank=nul) == E_ARG and find(Ls=0) == E_ARG and find(Ls=65) == E_ARG and find(B=-1) == E_ARG
    assert find(B=0) == OK
    with pytest.raises(polar_amd.PolarError):
        g.decode_scl_llr_list(np.zeros((2, 64)), 0)
    with pytest.raises(polar_amd.PolarError):
        g.decode_scl_llr_list(np.zeros((2, 64), np.float32), 4, fmt="bf16")
