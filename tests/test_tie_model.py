"""CPU suite: the list walk with the reference's tie rule (tests/tie_numpy.py) and the two classes of tie rows it tells apart.

Rows of ONE magnitude — sign(noisy codeword) * 45, what a hard-decision front end delivers — put almost every fork of the list walk
on a tie. The model must equal the oracle (and, where it was built, the unmodified reference) on every such row; a row is EXACTLY
DECIDED when the fp64 walk keeps, at every fork, the set that exact (a, k) metrics a + k log 2 keep under the same index rule. On
those rows the reference's answer follows from the rule alone, and tests/test_gpu_ties.py holds every decoder of the library to it.
The indices are stored in tests/golden/tie_rows.npz (tests/golden/make_tie_rows.py) and recomputed here.

The +-1 / +-3 rows of tests/test_gpu_r1_block.py::test_exact_zero_leaf_llrs are the other class: NOISE-DECIDED, some fork keeps
another set at 60 digits than in fp64. DESIGN.md §8 says that the seven rows on which the library differs from the oracle are of
that class; test_noise_class asserts it."""
import math

import numpy as np
import pytest

import oracle_lib
import tie_numpy as T

CODES = sorted(T.TIE_CODES)
ids = lambda c: "-".join(str(v) for v in c) if isinstance(c, tuple) else str(c)            # noqa: E731

TIE_ROWS_OFF_ORACLE_8_128_8 = (3, 6, 9, 14, 16, 17, 18)          # (tests/test_gpu_r1_block.py; asserted equal below)
AGREEING_ROWS = (0, 1, 2)


def test_keep_rule_by_hand():
    """PolarCode.cpp:521-553 on hand-made metrics: better than the threshold first, then equal ones by fork index."""
    c = T._cmp64
    assert T.keep_set([1.0, 1.0, 1.0, 1.0], 2, c) == {0, 1}
    assert T.keep_set([2.0, 1.0, 2.0, 0.5, None, None, 2.0, 3.0], 3, c) == {1, 3, 0}
    assert T.keep_set([math.inf, 0.0, math.inf, math.inf], 2, c) == {1, 0}
    assert T.keep_set([None, None, 5.0, 4.0], 2, c) == {2, 3}
    e = T._Exact()
    # 45 + 0 log 2 against 0 + 65 log 2 = 45.05...: the pair (45, 0) is smaller; equal pairs tie and go by index
    assert T.keep_set([(0.0, 65), (45.0, 0), (45.0, 0), (0.0, 65)], 2, e.cmp) == {1, 2}
    assert T.keep_set([(0.0, 65), (45.0, 0), (0.0, 65), (0.0, 65)], 2, e.cmp) == {1, 0}
    assert e.cmp((math.inf, 3), (math.inf, 0)) == 0 and e.cmp((1e6, 0), (math.inf, 0)) == -1


def test_exact_arithmetic_refuses_other_rows(oracle_built):
    o, c, x = T.case((8, 128, 8))
    with pytest.raises(T.NotExact):
        T.walk(c, x[0] / 45.0, 4, "exact")
    with pytest.raises(T.NotExact):
        T.walk(c, np.where(np.arange(c.N) == 7, 39.0, x[0]), 4, "exact")


@pytest.mark.parametrize("code", CODES, ids=ids)
def test_model_equals_oracle(oracle_built, code):
    """Every tie row at every list size the GPU tests use: the walk's word is the oracle's, and the stored bits are those."""
    o, c, x = T.case(code)
    gold = T.load_golden()
    assert (np.abs(x) == T.TIE_C).all() and len({tuple(r) for r in x}) == len(x)
    for L in T.TIE_CODES[code][1]:
        want = o.decode_scl_llr(x, L)
        got = np.stack([T.walked(code, L, r).info for r in range(len(x))])
        assert (got == want).all(), (L, np.nonzero((got != want).any(axis=1))[0])
        assert (gold[(code, L)][1] == want).all()
        for r in range(len(x)):                             # the returned word is a path of the final list, the winner's
            res = T.walked(code, L, r)
            assert [p["index"] for p in res.paths] == sorted(p["index"] for p in res.paths) and 1 <= len(res.paths) <= L
            w = [p for p in res.paths if p["index"] == res.winner]
            assert not w or (w[0]["info"] == res.info).all()


def test_model_equals_oracle_on_the_pm1_pm3_rows(oracle_built):
    """The 20 rows of test_exact_zero_leaf_llrs, (8, 128, 8), L = 1, 4, 32: here f is the libm expression, not min-sum."""
    o, c, _ = T.case((8, 128, 8))
    x = T.pm1_pm3_rows(o)
    assert set(np.abs(x[:10]).ravel()) == {1.0} and set(np.abs(x[10:]).ravel()) == {3.0}
    for L in (1, 4, 32):
        want = o.decode_scl_llr(x, L)
        got = np.stack([T.walk(c, x[r], L).info for r in range(20)])
        assert (got == want).all(), (L, np.nonzero((got != want).any(axis=1))[0])


@pytest.mark.skipif(not oracle_lib.have_reference(), reason="oracle/_ref not built here")
@pytest.mark.parametrize("code", CODES, ids=ids)
def test_model_equals_reference(oracle_built, code):
    import ctypes as C
    o, c, x = T.case(code)
    C.CDLL(None).srand(1)
    r = oracle_lib.Reference(code[0], code[1], 0.32, code[2])
    assert (r.frozen() == o.frozen()).all() and (r.crc_matrix() == o.crc_matrix()).all()
    for L in T.TIE_CODES[code][1]:
        want = r.decode_scl_llr(x, L)
        got = np.stack([T.walked(code, L, i).info for i in range(len(x))])
        assert (got == want).all(), (L, np.nonzero((got != want).any(axis=1))[0])


@pytest.mark.parametrize("code", CODES, ids=ids)
def test_exact_class(oracle_built, code):
    """At least half the committed rows of every (code, list size) are exactly decided — a cap on the choice of magnitude and
    seed, met by the reference alone — and the stored indices are the model's: all rows of the N = 256 and N = 512 codes, two
    rows per list size (one stored as exactly decided, where there is one that is not: one of those) at N = 1024."""
    gold = T.load_golden()
    rows = T.TIE_CODES[code][0]
    for L in T.TIE_CODES[code][1]:
        stored = gold[(code, L)][0]
        assert 2 * len(stored) >= rows and (np.diff(stored) > 0).all() and stored.min() >= 0 and stored.max() < rows
        if code[0] < 10:
            check = range(rows)
        else:
            others = [r for r in range(rows) if r not in stored]
            check = [int(stored[L % len(stored)]), others[0] if others else int(stored[(L + 3) % len(stored)])]
        for r in check:
            assert T.walked(code, L, r).exactly_decided() == (r in stored), (L, r)
        ties = [len(T.walked(code, L, r).tie_forks()) for r in check]
        print("%s L = %2d: %2d of %d rows exactly decided; forks with a tie at the cut per row: median %g of %d" %
              (ids(code), L, len(stored), rows, np.median(ties), code[1] + code[2]))


def test_noise_class(oracle_built):
    """DESIGN.md §8 as a test: each of the seven +-1 / +-3 rows of (8, 128, 8) that the library decodes differently from the oracle
    at L = 32 has a fork at which fp64 keeps another set than 60-digit arithmetic does (equal to 1e-40 = a tie, same index rule):
    the reference decides it on the rounding of its own sums. An agreeing row may be noise-decided too — the library's arithmetic
    then happens to round the same way, or the other set leads to the same word; three of them are walked for the record and
    nothing is asserted on them."""
    import test_gpu_r1_block
    assert test_gpu_r1_block.TIE_ROWS_OFF_ORACLE_8_128_8 == TIE_ROWS_OFF_ORACLE_8_128_8
    o, c, _ = T.case((8, 128, 8))
    x = T.pm1_pm3_rows(o)
    want = o.decode_scl_llr(x, 32)
    decided = {}
    for r in TIE_ROWS_OFF_ORACLE_8_128_8 + AGREEING_ROWS:
        res = T.walk(c, x[r], 32, "mp")
        assert (res.info == want[r]).all()
        f = res.first_difference()
        decided[r] = f is not None
        print("row %2d (%s): %s" % (r, "off the oracle" if r in TIE_ROWS_OFF_ORACLE_8_128_8 else "agrees",
                                    "no fork differs" if f is None else
                                    "first noise-decided fork at leaf %d (%d of %d forks kept), fp64 margin %s ulps; %d such forks" %
                                    (f.phi, f.rho, f.offered, f.margin_ulps(), sum(k.differs for k in res.forks))))
    assert all(decided[r] for r in TIE_ROWS_OFF_ORACLE_8_128_8), decided
