"""SCAN soft-output decoding, the part that needs no GPU: the numpy model the device is compared against (tests/scan_numpy.py) gives
the counts its shared inputs were chosen for, its rows meet the margin condition, its tolerance is what the CPU measurement gives, its
structural properties hold, and the three entry points check their arguments before they touch a device."""
import ctypes as C

import numpy as np
import pytest

import scan_numpy as M
import scl_list_numpy as S

E_ARG, E_UNSUPPORTED, OK = -1, -4, 0


@pytest.mark.parametrize("key,iters,err,undet,it_sum,err_e,undet_e", M.TABLE)
def test_table_rows(oracle_built, key, iters, err, undet, it_sum, err_e, undet_e):
    code, llr, sent, r = M.table_reference(key, iters)
    e = M.table_reference(key, iters, True)[3]
    assert len(llr) == 256
    c, ce = M.counters(r, sent, key[2]), M.counters(e, sent, key[2])
    print(key, iters, c.tolist(), ce.tolist(), "rows below MARGIN", int((M.row_margins(code, r) < M.MARGIN).sum()))
    assert c.tolist() == [256, err, undet, 256 * iters] and ce.tolist() == [256, err_e, undet_e, it_sum]
    assert (r["n_iter"] == iters).all() and (e["n_iter"] <= iters).all()
    # early stop: a row stops at the first iteration whose word passes, with that iteration's outputs; a row that never passes is the
    # call without the flag
    for it in range(1, iters + 1):
        at = e["n_iter"] == it
        full = M.table_reference(key, it)[3]
        assert (e["info"][at] == full["info"][at]).all() and (e["info_llr"][at] == full["info_llr"][at]).all()
        assert (e["ext"][at] == full["ext"][at]).all() and (it == iters or (e["crc_ok"][at] == 1).all())
        if it > 1:
            assert (M.table_reference(key, it - 1)[3]["crc_ok"][at] == 0).all()
    if key == (6, 32, 8) and iters == 4:
        assert np.bincount(e["n_iter"], minlength=5).tolist() == M.EARLY_HIST
        assert int(((e["n_iter"] == 4) & (e["crc_ok"] == 0)).sum()) == M.EARLY_NEVER


@pytest.mark.parametrize("key", M.CODES)
def test_structure(oracle_built, key):
    """ext is +inf exactly where the frozen set fixes a coded bit, under both arithmetics and at every iteration; nothing is NaN or
    -inf; out is the sign of info_llr; iterations do not depend on how many follow; the first iteration of an all-frozen-left node is
    SC's f."""
    _, code = M.code_of(key)
    llr = M.clean_rows(key, 16)[0]
    forced = M.forced_coded_bits(code)
    assert not forced.any()                 # (a constructed code leaves its last leaf unfrozen: no coded bit is fixed, ext is finite)
    for minsum in (False, True):
        r = M.decode(code, llr, 4, minsum=minsum)
        assert (np.isposinf(r["ext_all"]) == forced).all() and np.isfinite(r["ext_all"][:, :, ~forced]).all()
        assert np.isfinite(r["leaf"]).all()
        assert (r["info"] == (r["info_llr"] < 0)).all() and (r["n_iter"] == 4).all()
        r2 = M.decode(code, llr, 2, minsum=minsum)
        assert (r2["leaf"] == r["leaf"][:2]).all() and (r2["ext_all"] == r["ext_all"][:2]).all()
        # a decoded word never sets a frozen position: the decisions the outputs are read from are those of the unfrozen leaves alone
        u = S.word(code, r["info"], None)
        assert (u[:, code.frozen == 1] == 0).all()
    # the first leaf that is not frozen has, in iteration 1, the LLR SC gives it (everything before it is +inf, everything after it 0)
    import flip_numpy as F
    first = int(np.flatnonzero(code.frozen == 0)[0])
    r1 = M.decode(code, llr, 1)
    assert np.allclose(r1["leaf"][0][:, first], F.sc_pass(code, llr)[1][:, first], rtol=1e-9, atol=1e-12)


def _pruned_equals_unpruned(code, llr):
    unfrozen = code.frozen == 0
    for minsum in (False, True):
        leaf, ext = M.iterate(code, llr, 4, minsum)
        leaf_p, ext_p = M.pruned(code, llr, 4, minsum)
        assert np.array_equal(leaf[:, :, unfrozen], leaf_p[:, :, unfrozen]) and np.array_equal(ext, ext_p)


@pytest.mark.parametrize("key", M.CODES)
def test_the_kernels_walk_changes_no_value(oracle_built, key):
    """The kernel's schedule on the kernel's arrays (scan_numpy.pruned: no all-frozen subtree walked, constants for the B of all-frozen
    and all-unfrozen ones, one transient and one persistent B array) gives the unpruned recursion's leaf LLRs and ext, value for value."""
    _, code = M.code_of(key)
    rows = 8 if key[0] >= 10 else 32
    llr = np.concatenate([M.clean_rows(key, 64)[0][:rows], M.SCALE * M.plain_rows(key)[0][:rows], M.special_rows(key)])
    _pruned_equals_unpruned(code, llr)
    ops = M.schedule(code)
    assert all(lam < 16 and v < 65536 for _, lam, v, _, _, _ in ops)                  # (the fields of the op word)
    assert sum(1 for o in ops if o[0] == M.PAIR) <= code.N // 2 and ops[-1][:3] == ((M.PAIR if key[0] == 1 else M.UP), 0, 0)


def test_inf_pattern_of_a_code_with_a_frozen_tail():
    """A frozen set that fixes coded bits (the last leaves frozen — no construction does that): ext is +inf exactly there."""
    code = S.Code(M.TailTables())
    forced = M.forced_coded_bits(code)
    assert 0 < forced.sum() < 16
    llr = M.tail_rows()
    for minsum in (False, True):
        r = M.decode(code, llr, 4, minsum=minsum)             # (no MarginError on these rows)
        assert (np.isposinf(r["ext_all"]) == forced).all() and np.isfinite(r["ext_all"][:, :, ~forced]).all() and np.isfinite(r["leaf"]).all()
    _pruned_equals_unpruned(code, llr)


def test_all_zero_row_and_a_single_value(oracle_built):
    key = (5, 16, 8)
    _, code = M.code_of(key)
    x = M.special_rows(key)
    with pytest.raises(M.MarginError):
        M.decode(code, x[:1], 2)
    for minsum in (False, True):
        r = M.decode(code, x, 4, minsum=minsum, early_stop=True, check=False)
        fin = np.isfinite(r["ext"][0])
        assert (r["info"][0] == 0).all() and (r["info_llr"][0] == 0).all() and (r["ext"][0][fin] == 0).all()
        assert r["crc_ok"][0] == 1 and r["n_iter"][0] == 1
        assert not np.isnan(r["ext"]).any() and not np.isnan(r["info_llr"]).any()


def test_shared_rows_meet_the_margin(oracle_built):
    """No row of the shared inputs raises MarginError (decode() would), at any `iters` and with early stop; the early-stop rows hold
    rows that pass at once, later and never."""
    for key in M.CODES:
        _, code = M.code_of(key)
        for scale in (1.0, M.SCALE):
            llr, sent, trials = M.clean_rows(key, scale=scale)
            assert len(llr) == M.ROWS and (np.diff(trials) > 0).all()
            its, margin = (max(M.ITERS), M.MARGIN) if scale == 1.0 else (max(M.scaled_iters(key)), M.MARGIN_SCALED)
            r = M.decode(code, llr, its, early_stop=key[2] > 0, margin=margin)
            assert M.row_margins(code, r).min() >= margin
            if key[2] and scale == 1.0:
                h = np.bincount(r["n_iter"], minlength=5)
                print(key, h.tolist())
                assert h[1] > 0 and h[2] + h[3] > 0 and ((r["n_iter"] == 4) & (r["crc_ok"] == 0)).sum() > 0
    _, code = M.code_of((5, 16, 8))
    for B in M.EDGE_B:
        M.decode(code, M.clean_rows((5, 16, 8), B, seed=M.EDGE_SEED + B)[0], 4, early_stop=True)


def test_tol_is_what_the_cpu_measures(oracle_built):
    """The measurements behind TOL and TOL_SCALED, at a reduced row count: ten times the largest deviation stays below the constant,
    and the constant is within a factor ten of that."""
    for scaled, tol in ((False, M.TOL), (True, M.TOL_SCALED)):
        worst, per = M.measure_tol(rows=16, table_rows=32, edge=False, scaled=scaled)
        print("scaled" if scaled else "plain", "largest deviation %.3g, per code and iters %s, tolerance %.3g" %
              (worst, {k: "%.2g" % v for k, v in per.items()}, tol))
        assert 10 * worst <= tol <= 100 * worst
    assert M.MARGIN == 100 * M.TOL and M.MARGIN_SCALED == 100 * M.TOL_SCALED
    assert M.scaled_iters((7, 64, 8)) == M.ITERS and M.scaled_iters((10, 512, 8)) == M.scaled_iters((11, 1024, 16)) == (1, 2)


def test_abi_symbols_and_argument_checks(built_lib):
    import polar_amd
    L = polar_amd.lib()
    for name in ("polar_decode_scan_batch_dev", "polar_decode_scan_batch", "polar_mc_batch_scan"):
        assert hasattr(L, name), name
    assert polar_amd.SN_N == 4 and polar_amd.SCAN_MAX_ITERS == 32 and (polar_amd.SCAN_MINSUM, polar_amd.SCAN_EARLY_STOP) == (1, 2)
    g = polar_amd.PolarCode(6, 32, 0.32, 8)
    g0 = polar_amd.PolarCode(6, 32, 0.32, 0)
    g12 = polar_amd.PolarCode(*M.REFUSED[:2], 0.32, M.REFUSED[2])
    h = g._h
    buf = np.zeros(4096, np.uint8)
    p = C.c_void_p(buf.ctypes.data)            # (never dereferenced: every call below is refused or has B = 0 / T = 0)
    odd = C.c_void_p(buf.ctypes.data + 1)
    nul = C.c_void_p(0)

    def dev(h=h, llr=p, fmt=0, B=1, iters=4, flags=0, out=p):
        return L.polar_decode_scan_batch_dev(h, llr, C.c_int(fmt), C.c_long(B), C.c_int(iters), C.c_int(flags), out, nul, nul, nul, nul, nul)

    def host(h=h, llr=p, fmt=0, B=1, iters=4, flags=0, out=p):
        return L.polar_decode_scan_batch(h, llr, C.c_int(fmt), C.c_long(B), C.c_int(iters), C.c_int(flags), out, nul, nul, nul, nul)

    for f in (dev, host):
        assert f(h=nul) == E_ARG and f(llr=nul) == E_ARG and f(out=nul) == E_ARG
        assert f(iters=0) == E_ARG and f(iters=33) == E_ARG and f(iters=-1) == E_ARG
        assert f(flags=4) == E_ARG and f(flags=-1) == E_ARG and f(flags=8 | 1) == E_ARG
        assert f(fmt=-1) == E_ARG and f(fmt=4) == E_ARG
        assert f(llr=odd, fmt=2) == E_ARG and f(llr=odd, fmt=3) == E_ARG
        assert f(B=-1) == E_ARG
        assert f(h=g0._h, flags=2) == E_ARG and f(h=g0._h, flags=3, B=0) == E_ARG           # no CRC: nothing to stop on
        assert f(h=g0._h, B=0) == OK and f(h=g0._h, B=0, flags=1) == OK
        assert f(B=0) == OK and f(B=0, iters=1) == OK and f(B=0, iters=32, flags=3, fmt=3) == OK
        assert f(h=g12._h) == E_UNSUPPORTED and f(h=g12._h, B=0) == E_UNSUPPORTED and f(h=g12._h, iters=33) == E_ARG
    assert dev(iters=33) == E_ARG and b"iters" in L.polar_last_error()
    assert dev(flags=4) == E_ARG and b"flag" in L.polar_last_error()

    axis = np.array([1.5, 2.0])
    en = np.ones(2, np.uint8)
    stats = np.zeros((2, 4), np.uint64)

    def mc(h=h, const=0, T=1, stride=1, ax=C.c_void_p(axis.ctypes.data), n_e=2, iters=4, flags=0, en=C.c_void_p(en.ctypes.data),
           st=C.c_void_p(stats.ctypes.data)):
        return L.polar_mc_batch_scan(h, C.c_int(const), C.c_uint64(1), C.c_uint64(0), C.c_long(T), C.c_long(stride), ax, C.c_int(n_e),
                                     C.c_int(iters), C.c_int(flags), en, st)

    assert mc(h=nul) == E_ARG and mc(ax=nul) == E_ARG and mc(en=nul) == E_ARG and mc(st=nul) == E_ARG
    assert mc(const=polar_amd.RX_MLC | polar_amd.ASK4_SP) == E_ARG and mc(const=99) == E_ARG
    assert mc(T=-1) == E_ARG and mc(stride=0) == E_ARG and mc(n_e=0) == E_ARG
    assert mc(iters=0) == E_ARG and mc(iters=33) == E_ARG and mc(flags=4) == E_ARG
    assert mc(h=g0._h, flags=2) == E_ARG and mc(h=g12._h) == E_UNSUPPORTED
    assert mc(T=0) == OK and mc(T=0, const=polar_amd.ASK4_GRAY, iters=1, flags=3) == OK and mc(h=g0._h, T=0, flags=1) == OK
    assert (stats == 0).all()

    # the Python mirror passes its arguments on to the library
    for bad in (0, 33):
        with pytest.raises(polar_amd.PolarError):
            g.decode_scan(np.zeros((1, 64)), bad)
    with pytest.raises(polar_amd.PolarError):
        g0.decode_scan(np.zeros((1, 64)), 4, early_stop=True)
    with pytest.raises(polar_amd.PolarError, match="-4"):
        g12.decode_scan(np.zeros((1, 4096)), 4)
    with pytest.raises(polar_amd.PolarError):
        g.decode_scan(np.zeros((2, 64), np.float32), 4, fmt="bf16")
    with pytest.raises(polar_amd.PolarError):
        g.mc_batch_scan(1, 0, 0, 1, axis, 4, en, np.zeros((2, 6), np.uint64))       # stats of the wrong shape
    with pytest.raises(polar_amd.PolarError):
        g.scan_stats(axis, 4, max_runs=0)
