"""Rate-1 quads finished in one step by the list-of-32 kernels (polar_amd/csrc/polar_scl_leaf.inc): the host marks the
aligned blocks of four unfrozen leaves in the control words, and a wave whose first leaf of such a block takes the exact fast path
tries the other three at once. Every decode here is compared bit for bit with the CPU oracle AND with the same call under the knob
"no_r1" (control words without the marks: every leaf a loop step of its own); path metrics must be the same doubles in both.
Small batches: B = 1, 2, 3 and 40 — an odd B leaves a wave with one valid codeword.

The module runs on the test build of the library, whose list-of-32 units count the continuations of a launch (polar_debug_get
"r1_committed" / "r1_discarded"): wherever the CPU model of tests/r1_model.py can follow the decode, the two counts must equal the
model's, and the uploaded control words must carry the marks the model's statement of the host rule gives. On every input the
model has been run on (three codes, -8 .. 6 dB, L = 17 and 32: several thousand continuations) it gives up none: once the first
leaf of a rate-1 quad is fast, each g-node below adds the magnitudes of its operands, the later leaves are more reliable than the
first and pass as well, and a leaf LLR of exactly 0 cannot follow a fast first leaf (it needs a zero operand, which makes the first
leaf 0 and not fast). "discarded" is therefore asserted to be the model's 0, "committed" the model's positive count."""
import ctypes as C
import warnings

import numpy as np
import pytest

import r1_model

pytestmark = pytest.mark.gpu

_cache = {}


def rows(o, seed, B, snrs):
    """B rows, split evenly over the Eb/N0 points `snrs` (a low one: most blocks are given up; a high one: most are finished)"""
    parts, at = [], 0
    for i, s in enumerate(snrs):
        nb = (B - at) if i == len(snrs) - 1 else B // len(snrs)
        parts.append(o.synth_llr(seed, at, nb, o.snr_sqrt_linear(s))[0])
        at += nb
    return np.concatenate(parts)


def setup(code, B=40, snrs=(0.0, 4.0)):
    """-> (oracle, handle, llr rows [B, N]), once per code"""
    if code not in _cache:
        import polar_amd
        from oracle_lib import Oracle
        n, K, crc = code
        o = Oracle(n, K, 0.32, crc, srand=1)
        C.CDLL(None).srand(C.c_uint(1))
        g = polar_amd.PolarCode(n, K, 0.32, crc)
        _cache[code] = (o, g, rows(o, 777, B, snrs))
    return _cache[code]


def decode(g, llr, L, no_r1, knobs=None):
    import torch
    B = llr.shape[0]
    d_llr = torch.from_numpy(np.ascontiguousarray(llr)).cuda()
    out = torch.full((B, g.K), 7, dtype=torch.uint8, device="cuda")
    pm = torch.zeros(B, dtype=torch.float64, device="cuda")
    knobs = dict(knobs or {})
    knobs["no_r1"] = 1 if no_r1 else 0
    for k, v in knobs.items():
        g.debug_set(k, v)
    try:
        g.decode_scl_llr_dev(d_llr.data_ptr(), B, L, out.data_ptr(), pm_ptr=pm.data_ptr())
        torch.cuda.synchronize()
        g.r1_counts = (g.debug_get("r1_committed"), g.debug_get("r1_discarded"))       # (of this call's list-of-32 launch)
    finally:
        for k in knobs:
            g.debug_set(k, 0)
    return out.cpu().numpy(), pm.cpu().numpy()


def frozen_of(o):
    return np.asarray(o.frozen(), np.uint8)


def check_marks(o, g):
    """The uploaded control words against the model's statement of the host rule; -> rb per leaf."""
    fr = frozen_of(o)
    weak = r1_model.weak_leaves(fr)
    rb = r1_model.marks(fr, weak)
    marked, plain = g.debug_ctl_words(True), g.debug_ctl_words(False)
    assert ((marked >> 9) == rb).all(), np.nonzero((marked >> 9) != rb)[0][:10]
    assert (plain == (marked & 0x1FF)).all() and ((plain & 1) == fr).all() and (((plain >> 8) & 1) == weak).all()
    return rb


def both_ways(o, g, llr, L, knobs=None, want=None, model=True):
    """model: True = the launch's counters must equal the CPU model's counts (and something must have been committed);
    False = inputs the model cannot follow (metric ties): the continuation must at least have run."""
    want = o.decode_scl_llr(llr, L) if want is None else want
    bits, pm = decode(g, llr, L, False, knobs)
    got = g.r1_counts
    bits1, pm1 = decode(g, llr, L, True, knobs)
    assert g.r1_counts == (0, 0)                            # no marks: the continuation never starts
    if model:
        assert got == r1_model.counts(frozen_of(o), llr, L), got
    if model is False or (model and llr.shape[0] >= 8):
        assert got[0] > 0, got
    assert (bits == want).all(), np.nonzero((bits != want).any(axis=1))[0][:10]
    assert (bits1 == want).all(), np.nonzero((bits1 != want).any(axis=1))[0][:10]
    assert (pm.view(np.uint64) == pm1.view(np.uint64)).all(), np.nonzero(pm != pm1)[0][:10]
    return want


# ---- the generic-N object: no tables, no head
@pytest.mark.parametrize("code", ((8, 128, 8), (9, 128, 8)), ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("tuning", (0, 16))
def test_generic_n(hooks_lib, oracle_built, code, tuning):
    o, g, llr = setup(code)
    assert g.debug_get("test_hooks") == 1
    rb = check_marks(o, g)
    assert (rb == 3).sum() > 0 and (rb == 2).sum() > (rb == 3).sum()          # octets, and quads outside octets
    g.set_tuning(waves_per_cu=tuning)
    try:
        want = both_ways(o, g, llr, 32)
        for B in (1, 2, 3):
            both_ways(o, g, llr[40 - B:], 32, want=want[40 - B:])
            both_ways(o, g, llr[:B], 32, want=want[:B])
    finally:
        g.set_tuning(waves_per_cu=0)
    assert len({tuple(r[:32]) for r in want}) > 1


@pytest.mark.parametrize("L", (17, 24, 31))
def test_list_sizes_below_the_group(hooks_lib, oracle_built, L):
    """Lanes >= L are never active: a full list is nact == L."""
    for code in ((8, 128, 8), (9, 128, 8)):
        o, g, llr = setup(code)
        both_ways(o, g, np.concatenate([llr[:7], llr[-8:]]), L)


def test_high_rate_block_before_the_list_is_full(hooks_lib, oracle_built):
    """A rate-1 block that comes while the list still grows must never start the continuation: the model counts only blocks whose
    first leaf finds the list full. (6, 48, 0): the first marked block starts at the sixth unfrozen leaf — just full. An explicit
    mask at N = 64 whose FIRST unfrozen leaves are the marked quad [28, 32): one path there; the counts are the model's, which are
    the same with that mark taken away."""
    o, g, llr = setup((6, 48, 0), B=21, snrs=(1.0, 6.0))
    check_marks(o, g)
    both_ways(o, g, llr, 32)
    both_ways(o, g, llr[:1], 32)
    key = ("explicit", "early-quad")
    if key not in _cache:
        import polar_amd
        from oracle_lib import Oracle
        frozen = np.ones(64, np.uint8)
        frozen[28:32] = 0
        frozen[40:64] = 0
        K = int((frozen == 0).sum())
        order = np.concatenate([np.nonzero(frozen == 0)[0], np.nonzero(frozen)[0]]).astype(np.uint16)
        o = Oracle(6, K, 0.32, 0, srand=1)
        o.set_tables(frozen, order)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            g = polar_amd.PolarCode.from_tables(6, K, 0, frozen, order)
        _cache[key] = (o, g, rows(o, 99, 21, (2.0, 6.0)))
    o, g, llr = _cache[key]
    rb = check_marks(o, g)
    assert rb[28] == 2 and rb[40] == 3
    both_ways(o, g, llr, 32)
    rb0 = rb.copy()
    rb0[28] = 0
    assert r1_model.counts(frozen_of(o), llr, 32, rb0) == r1_model.counts(frozen_of(o), llr, 32, rb)


# ---- the fixed-N objects: table mode and the two-phase form (units 2 and 6)
HEAD_PHI = {(10, 512, 16): 0, (10, 256, 8): 368, (11, 1024, 16): 432}       # hand-over leaf of the two-phase form (0: window too short, one phase)


@pytest.mark.parametrize("code", sorted(HEAD_PHI), ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("form", ("tables", "no_tables", "head", "no_head"))
def test_fixed_n(hooks_lib, oracle_built, code, form):
    o, g, llr = setup(code, snrs=(1.0, 3.0))
    if ("want", code) not in _cache:
        _cache[("want", code)] = o.decode_scl_llr(llr, 32)
    want = _cache[("want", code)]
    knobs = {"tables": {}, "no_tables": {"no_tables": 1}, "head": {"head_min_b": 1}, "no_head": {"head_min_b": 1, "no_head": 1}}[form]
    g.set_tuning(waves_per_cu=16 if "head" in form else 0)
    try:
        check_marks(o, g)
        both_ways(o, g, llr, 32, knobs, want=want, model=False)
        assert g.debug_get("head_phi") == (HEAD_PHI[code] if form == "head" else 0)
        both_ways(o, g, llr[37:], 32, knobs, want=want[37:])          # (three rows: a wave with one valid codeword; counts = the model's)
    finally:
        g.set_tuning(waves_per_cu=0)


# ---- explicit masks (from_tables), N = 512, no CRC: unfrozen runs placed by hand.
#   name: (unfrozen leaves, what it exercises)
def _run(a, b):
    return list(range(a, b))


EXPLICIT = {
    # 25 unfrozen leaves, then the octet [448, 456): its 7th leaf is the 32nd unfrozen step -> the octet and its second quad are
    # not marked, the first quad is
    "flush-inside-octet": (_run(423, 448) + _run(448, 456) + _run(480, 512), "block shrunk by the host"),
    # 24 before: the octet's LAST leaf is the 32nd step -> marked, the history word is flushed right after the block
    "flush-after-octet": (_run(424, 448) + _run(448, 456) + _run(480, 512), "flush after the block"),
    # 28 before a quad whose last leaf is the 32nd step, and the mask ends in an octet at N - 1
    "flush-after-quad": (_run(404, 432) + _run(432, 436) + _run(496, 512), "flush after a quad; block ending at leaf N - 1"),
    # a quad and an octet in channels no construction would use (weak leaves: never marked) once the list is full
    "weak-block": (_run(96, 104) + _run(128, 132) + _run(136, 144) + _run(448, 512), "blocks containing weak leaves"),
}


def explicit_setup(name, B=24):
    key = ("explicit", name)
    if key not in _cache:
        import polar_amd
        from oracle_lib import Oracle
        n, N = 9, 512
        frozen = np.ones(N, np.uint8)
        frozen[EXPLICIT[name][0]] = 0
        K = int((frozen == 0).sum())
        order = np.concatenate([np.nonzero(frozen == 0)[0], np.nonzero(frozen)[0]]).astype(np.uint16)
        o = Oracle(n, K, 0.32, 0, srand=1)
        o.set_tables(frozen, order)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")              # (hand-placed leaves: the weak-leaves warning is expected)
            g = polar_amd.PolarCode.from_tables(n, K, 0, frozen, order)
        _cache[key] = (o, g, rows(o, 99, B, (2.0, 6.0)))
    return _cache[key]


# the marks each mask must get, stated by hand: {leaf: rb} for every leaf of the runs named in the comment above; all others 0
EXPECT_RB = {
    # (the run [480, 512) starts at t = 33: leaf 510 is the 64th unfrozen step, so the octet [504, 512) shrinks to its first quad)
    "flush-inside-octet": {448: 2, 480: 3, 484: 2, 488: 3, 492: 2, 496: 3, 500: 2, 504: 2,
                           424: 3, 428: 2, 432: 3, 436: 2, 440: 3, 444: 2},
    "flush-after-octet": {448: 3, 452: 2, 480: 3, 484: 2, 488: 3, 492: 2, 496: 3, 500: 2, 504: 3, 508: 2,
                          424: 3, 428: 2, 432: 3, 436: 2, 440: 3, 444: 2},
    "flush-after-quad": {432: 2, 496: 3, 500: 2, 504: 3, 508: 2,
                         404: 2, 408: 3, 412: 2, 416: 3, 420: 2, 424: 3, 428: 2},
}


@pytest.mark.parametrize("name", sorted(EXPLICIT))
def test_explicit_masks(hooks_lib, oracle_built, name):
    o, g, llr = explicit_setup(name)
    rb = check_marks(o, g)
    if name in EXPECT_RB:
        assert {int(i): int(rb[i]) for i in np.nonzero(rb)[0]} == EXPECT_RB[name]
    else:
        # the quad [128, 132) is four weak leaves, the octet [136, 144) has seven: neither is marked, nor any of its quads; no
        # marked block anywhere holds a weak leaf
        weak = r1_model.weak_leaves(frozen_of(o))
        assert weak[128:132].all() and weak[136:143].all() and not rb[:448].any() and rb[448] == 3
        for i in np.nonzero(rb)[0]:
            assert not weak[i:i + (1 << rb[i])].any()
    want = both_ways(o, g, llr, 32)
    both_ways(o, g, llr[:3], 32, want=want[:3])
    assert len({tuple(r[:16]) for r in want}) > 1


def test_block_at_the_hand_over_leaf(hooks_lib, oracle_built):
    """An octet that starts AT the hand-over leaf of the two-phase form (N = 1024: unfrozen 255, 383, then [496, 504), a
    Bhattacharyya code's leaves from 512 on; hand-over 496 = the third unfrozen leaf): the layers of size 4 and 2 of its quads come
    from the walk that starts at the import. Two unfrozen leaves lie before the hand-over by construction (it is the largest
    multiple of 16 not above the THIRD), so a list of 17 .. 32 is never full there: the marked block at the hand-over leaf is
    never tried — the model's counts are the same with that mark taken away — and the device's counts equal the model's."""
    key = ("explicit", "hand-over")
    if key not in _cache:
        import polar_amd
        from oracle_lib import Oracle
        n, N = 10, 1024
        frozen = np.ones(N, np.uint8)
        frozen[512:] = np.asarray(Oracle(n, 512, 0.32, 16).frozen(), np.uint8)[512:]
        frozen[[255, 383]] = 0
        frozen[496:504] = 0
        K = int((frozen == 0).sum())
        order = np.concatenate([np.nonzero(frozen == 0)[0], np.nonzero(frozen)[0]]).astype(np.uint16)
        o = Oracle(n, K, 0.32, 0, srand=1)
        o.set_tables(frozen, order)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            g = polar_amd.PolarCode.from_tables(n, K, 0, frozen, order)
        _cache[key] = (o, g, rows(o, 99, 12, (1.0, 3.0)))
    o, g, llr = _cache[key]
    rb = check_marks(o, g)
    assert rb[496] == 3 and rb[500] == 2
    g.set_tuning(waves_per_cu=16)
    try:
        both_ways(o, g, llr, 32, {"head_min_b": 1})
        assert g.debug_get("head_phi") == 496
        rb0 = rb.copy()
        rb0[496] = 0
        assert r1_model.counts(frozen_of(o), llr, 32, rb0) == r1_model.counts(frozen_of(o), llr, 32, rb)
    finally:
        g.set_tuning(waves_per_cu=0)


# ---- values
@pytest.mark.parametrize("scale", (30.0, 300.0))
def test_l_form_values_and_underflowing_products(hooks_lib, oracle_built, scale):
    """Rows scaled so that |x| >= 690 (L-form) and g products below e^-690 occur inside the blocks. The saturated metrics tie, so
    the CPU model cannot follow these rows. x 30: the continuation must have run (committed > 0). x 300: every leaf is beyond the
    range where the logarithms differ from |x|, good and bad forks tie and no leaf step is fast — no count is asserted there."""
    o, g, llr = setup((9, 128, 8))
    both_ways(o, g, llr[10:31] * scale, 32, model=False if scale == 30.0 else None)


# rows of the (8, 128, 8) tie set below that differ from the oracle in the library with and without the continuation, on the host
# path too (every metric of such a row ties; the reference decides them on the rounding noise of its own arithmetic): a divergence
# of the library that predates the rate-1 blocks, recorded in DESIGN.md §8 "Out of scope / not done"
TIE_ROWS_OFF_ORACLE_8_128_8 = (3, 6, 9, 14, 16, 17, 18)


def test_exact_zero_leaf_llrs(hooks_lib, oracle_built):
    """Rows of +-1 and +-3 with the signs of noisy codewords: g-nodes whose operands cancel give LLR 0 exactly — a stored value of
    magnitude 1.0, which decides 0 whatever its sign bit. Every metric of such a row ties, so the CPU model cannot follow it and no
    count is asserted; bits against the oracle, bits and metrics against no_r1."""
    o, g, llr = setup((9, 128, 8))
    sg = np.where(llr[:20] < 0, -1.0, 1.0)
    both_ways(o, g, np.concatenate([sg[:10], 3.0 * sg[10:]]), 32, model=None)
    o, g, llr = setup((8, 128, 8))
    sg = np.where(llr[:20] < 0, -1.0, 1.0)
    x = np.concatenate([sg[:10], 3.0 * sg[10:]])
    want = o.decode_scl_llr(x, 32)
    bits, pm = decode(g, x, 32, False)
    bits1, pm1 = decode(g, x, 32, True)
    agree = np.array([i for i in range(20) if i not in TIE_ROWS_OFF_ORACLE_8_128_8])
    assert (bits[agree] == want[agree]).all() and (bits1[agree] == want[agree]).all()
    assert (bits == bits1).all() and (pm.view(np.uint64) == pm1.view(np.uint64)).all()


def test_knob_switched_on_one_handle(hooks_lib, oracle_built):
    """no_r1 on, off and on again on one handle, a smaller batch in between: nothing is left behind."""
    o, g, llr = setup((11, 1024, 16), snrs=(1.0, 3.0))
    if ("want", (11, 1024, 16)) not in _cache:
        _cache[("want", (11, 1024, 16))] = o.decode_scl_llr(llr, 32)
    want = _cache[("want", (11, 1024, 16))]
    for no_r1, sl in ((True, slice(0, 40)), (False, slice(0, 40)), (True, slice(20, 37)), (False, slice(3, 9)), (True, slice(0, 40))):
        bits, _ = decode(g, llr[sl], 32, no_r1)
        assert (bits == want[sl]).all()
