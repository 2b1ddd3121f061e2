"""CPU suite: what tests/test_gpu_masks.py rests on, proven on the oracle and numpy alone — the coverage of the masks of
tests/mask_cases.py (every mixed octet and quad pattern, the pair (unfrozen, frozen)), that none of them is an up-set of the bitwise
order or has a weak unfrozen leaf, the conditions on the rows, and that the oracle with explicit tables and the numpy SC pass state
the same decoder on them. If a condition fails, move a seed or an Eb/N0 point in mask_cases.py; no GPU assertion is widened."""
import numpy as np
import pytest

import guard_numpy as G
import mask_cases as MC
import scl_list_numpy as S
from r1_model import weak_leaves


def _all_tables():
    return MC.octet_codes(11) + MC.octet_codes(10) + list(MC.edge_masks().values())


def test_a_constructed_mask_has_18_mixed_octet_patterns(oracle_built):
    """The argument of DESIGN.md on the bases themselves: up-sets, whose octets show none but the 20 up-set patterns of three bits,
    whose quads none but 6, and never the pair (unfrozen, frozen)."""
    ups8 = {p for p in range(256) if MC.is_up_set([(p >> j) & 1 for j in range(8)])}
    ups4 = {p for p in range(16) if MC.is_up_set([(p >> j) & 1 for j in range(4)])}
    assert len(ups8) == 20 and len(ups8 - {0, 255}) == 18 and len(ups4) == 6
    for n in (7, 10, 11):
        base = MC.base_frozen(n)
        assert MC.is_up_set(base)
        assert set(MC.octet_patterns(base).tolist()) <= ups8 and set(MC.quad_patterns(base).tolist()) <= ups4
        assert not ((base[0::2] == 0) & (base[1::2] == 1)).any()


def test_coverage(oracle_built):
    """254 / 14 / 1: every mixed octet pattern in each of the two sets, every mixed quad pattern and the pair in the n = 10 set."""
    mixed8, mixed4 = set(range(1, 255)), set(range(1, 15))
    for n in (11, 10):
        codes = MC.octet_codes(n)
        seen8 = set().union(*[set(MC.octet_patterns(t.frozen()).tolist()) for t in codes]) & mixed8
        seen4 = set().union(*[set(MC.quad_patterns(t.frozen()).tolist()) for t in codes]) & mixed4
        pair = sum(int(((t.frozen()[0::2] == 0) & (t.frozen()[1::2] == 1)).sum()) for t in codes)
        new8 = seen8 - set(MC.octet_patterns(MC.base_frozen(n)).tolist())
        print("n = %d: %d codes, %d mixed octet patterns (%d of them in no constructed mask), %d mixed quad patterns, the pair "
              "(unfrozen, frozen) %d times" % (n, len(codes), len(seen8), len(new8), len(seen4), pair))
        assert seen8 == mixed8 and seen4 == mixed4 and pair > 0
        assert len(new8) >= 236


def test_masks_are_no_up_sets_and_have_no_weak_leaf(oracle_built):
    for t in _all_tables():
        f = t.frozen()
        assert not MC.is_up_set(f), t
        assert weak_leaves(f).sum() == 0, t
        base = MC.base_frozen(t.n)
        assert (f >= base).all() and (f != base).any(), t                      # (leaves are frozen, none is set free)
        assert t.K == int((f == 0).sum()) and sorted(t.order().tolist()) == list(range(t.N))
        c = t.with_crc()
        assert c.K == t.K - MC.CRC and c.crc_matrix().shape == (MC.CRC, c.K)
        assert not f[c.order()[:c.K + c.crc]].any() and f[c.order()[c.K + c.crc:]].all()


def test_edge_masks_are_what_their_names_say(oracle_built):
    e, base = MC.edge_masks(), MC.base_frozen(10)
    assert len(e) == 11 and all(t.N <= 1024 for t in e.values())
    assert e["a-last-leaf"].frozen()[-1] == 1 and not e["a-last-leaf"].frozen()[-8:-1].any()
    assert e["a-last-quad"].frozen()[-4:].all() and not e["a-last-quad"].frozen()[-8:-4].any()
    for half in (16, 64):
        f = e["b-right-half-%d" % half].frozen()
        b = int(np.flatnonzero((f != base).reshape(-1, half).any(axis=1))[0])
        assert b & 1 and f[b * half:(b + 1) * half].all() and not f[(b - 1) * half:b * half].all()
        assert (f != base).sum() == half
    o = MC.straddling_octet(base)
    for pos in (1, 2, 5, 7):
        f = e["c-leaf-%d" % pos].frozen()
        assert MC.octet_patterns(f)[o] == 1 << pos and (f != base).sum() == 1
        t = np.cumsum(f == 0) - 1                                             # the decision count of every unfrozen leaf
        mine = [i for i in range(8 * o, 8 * o + 8) if not f[i]]
        assert any((t[i] & 31) == 31 for i in mine[:-1]), pos                 # a history word is flushed inside the octet
    assert MC.quad_patterns(e["c-leaf-2"].frozen())[2 * o] == 4 and MC.quad_patterns(e["c-leaf-5"].frozen())[2 * o + 1] == 2
    assert len(MC.n128_masks()) == 3 and all(t.N == 128 for t in MC.n128_masks())


@pytest.mark.parametrize("n", [11, 10])
def test_row_conditions(oracle_built, n):
    """Every octet-pattern code keeps at least 3/4 of its rows; among them the oracle's list-size-1 decode has a block error and a
    correct block."""
    for t in MC.octet_codes(n):
        r = MC.rows(t)
        k = r.keep_l1
        print(t, "kept", int(k.sum()), "of", len(k), "(list kernels:", int(r.keep_list.sum()), ") block errors", int(r.err_l1[k].sum()),
              "largest all-frozen sum %.0f" % r.fsum.max(), "smallest product %.2g" % r.prod.min())
        assert 4 * k.sum() >= 3 * len(k) and 4 * r.keep_list.sum() >= 3 * len(k), t
        assert r.err_l1[k].any() and (~r.err_l1[k]).any(), t
        assert (r.prod[k] >= MC.PROD_MIN).all() and (r.fsum[k] <= MC.FSUM_MAX).all() and (r.win[k] >= MC.WINDOW).all()


def test_edge_mask_rows(oracle_built):
    """The edge masks go through the list kernels, whose criteria are those on the input and the window: at least 3/4 of the rows stay,
    with block errors among them at list size 1."""
    for t in MC.edge_masks().values():
        r = MC.rows(t)
        assert 4 * r.keep_list.sum() >= 3 * len(r.keep_list), t
        assert r.err_l1[r.keep_list].any() and (~r.err_l1[r.keep_list]).any(), t


def test_oracle_and_numpy_sc_agree(oracle_built):
    """The oracle with set_tables against flip_numpy.sc_pass and guard_numpy.sc_decisions, and the vectorised margins against
    guard_numpy.l1_margins, on the kept rows (the scalar functions on a few rows per code: they take a second per row at N = 2048)."""
    for t in _all_tables():
        r = MC.rows(t)
        k = np.flatnonzero(r.keep_list)
        assert np.array_equal(S.split(r.code, r.u)[0][k], r.bits_l1[k]), t
        for i in k[[0, len(k) // 2, -1]]:
            u = G.sc_decisions(r.code, r.llr[i])
            assert np.array_equal(u, r.u[i]), (t, i)
            prod, fsum, zero, win = G.l1_margins(r.code, r.llr[i], u)
            assert (prod, fsum, zero, win.min()) == (r.prod[i], r.fsum[i], r.zero[i], r.win[i]), (t, i)
        # a CRC changes neither the mask nor the pass: the variant's oracle decodes the same leaves
        c = t.with_crc()
        assert np.array_equal(c.frozen(), t.frozen())


def test_flip_and_scan_rows(oracle_built):
    """The rows of the SC-Flip and SCAN comparisons: the numpy models refuse none of them (MarginError), both outcomes of the CRC
    occur, and retries deliver words."""
    import flip_numpy as F
    import scan_numpy as M
    codes = MC.soft_codes()
    assert len(codes) == len(MC.octet_codes(10)) + 6
    first = flipped = 0
    for t in codes:
        code = S.Code(t)
        llr, sent = MC.flip_rows(t)
        assert len(llr) == MC.FLIP_ROWS
        r = F.decode(code, llr, max(MC.FLIP_T))
        first, flipped = first + F.shares(r)[0], flipped + F.shares(r)[1]
    assert first > 0 and flipped > 0
    for t in MC.scan_codes():
        plain, clean = MC.scan_rows(t)
        assert len(plain) == len(clean) == MC.SCAN_ROWS, t
    for t in codes[:2]:                                                        # (the GPU test runs the model on every code)
        M.decode(S.Code(t), MC.scan_rows(t)[1], max(M.ITERS), margin=MC.SCAN_MARGIN)


def test_scan_tolerance_is_the_measured_one(oracle_built):
    """SCAN_TOL is ten times the largest deviation measure_scan_tol found; one draw over four codes here stays below a tenth of it."""
    codes = MC.soft_codes()
    d = MC.measure_scan_tol(draws=(0,), codes=[codes[0], codes[5], codes[-6], codes[-1]])
    print("largest deviation of the perturbed model %.3g, SCAN_TOL %.3g" % (d, MC.SCAN_TOL))
    assert d <= MC.SCAN_TOL / 10


def test_whole_list_rows(oracle_built):
    """N = 128: scl_list raises TieError on at most 1/4 of the rows of a mask, at list sizes 4 and 8."""
    for t in MC.n128_masks():
        llr, sent, lists, kept = MC.list_rows(t, (4, 8))
        print(t, "rows without a tie", len(kept), "of", len(llr))
        assert 4 * len(kept) >= 3 * len(llr), t
    # the adaptive comparison: the same bound, and every stage of the schedule delivers a row
    import adaptive_numpy as A
    t = MC.adaptive_case()
    llr, _, _, kept = MC.list_rows(t, MC.ADAPTIVE)
    assert t.N == 128 and t.crc == MC.CRC and 4 * len(kept) >= 3 * len(llr)
    _, _, stage, ok = A.adaptive(S.Code(t), llr[kept], MC.ADAPTIVE)
    print(t, "rows without a tie", len(kept), "stages", np.bincount(stage, minlength=3).tolist(), "accepted", int(ok.sum()))
    assert len(set(stage.tolist())) == 3 and ok.sum() > 0


def test_collection_constants(oracle_built):
    """What tests/test_gpu_masks.py is parametrised by without building anything."""
    assert {n: len(MC.octet_codes(n)) for n in (11, 10)} == MC.N_CODES
    assert tuple(MC.edge_masks()) == MC.EDGE_NAMES
    assert len(MC.soft_codes()) == MC.N_SOFT and len(MC.scan_codes()) == MC.N_SOFT + 2
    assert len({t.seed for t in MC.octet_codes(11) + MC.octet_codes(10)}) == 20
