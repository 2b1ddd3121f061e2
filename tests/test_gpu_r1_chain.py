"""The two sequels of the rate-1 quad continuation of the list-of-32 kernels (polar_amd/csrc/polar_scl_leaf.inc): the
continuation entered after a first leaf that took the ranking path with the list full, and the second quad of a marked octet finished
in the step that finished the first. The cases are those of tests/test_gpu_r1_block.py: every decode is compared bit for bit with the
CPU oracle AND with the same call under the knob "no_r1" (bits, and path metrics as the same doubles); wherever the CPU model of
tests/r1_chain_model.py can follow the decode, the six counters of the test library (polar_debug_get "r1_committed", "r1_discarded",
"r1_rank_tried", "r1_rank_committed", "r1_chain_tried", "r1_chain_committed") must equal the model's."""
import ctypes as C
import warnings

import numpy as np
import pytest

import r1_chain_model
import r1_model

pytestmark = pytest.mark.gpu

NAMES = ("r1_committed", "r1_discarded", "r1_rank_tried", "r1_rank_committed", "r1_chain_tried", "r1_chain_committed")
_cache = {}


def rows(o, seed, B, snrs):
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


def from_mask(key, n, unfrozen, B, seed=99, snrs=(2.0, 6.0)):
    """-> (oracle, handle, llr rows) of an explicit frozen mask (no CRC), once per key"""
    if key not in _cache:
        import polar_amd
        from oracle_lib import Oracle
        frozen = np.ones(1 << n, np.uint8)
        frozen[unfrozen] = 0
        K = int((frozen == 0).sum())
        order = np.concatenate([np.nonzero(frozen == 0)[0], np.nonzero(frozen)[0]]).astype(np.uint16)
        o = Oracle(n, K, 0.32, 0, srand=1)
        o.set_tables(frozen, order)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")              # (hand-placed leaves: the weak-leaves warning is expected)
            g = polar_amd.PolarCode.from_tables(n, K, 0, frozen, order)
        _cache[key] = (o, g, rows(o, seed, B, snrs))
    return _cache[key]


def decode(g, llr, L, no_r1, knobs=None):
    """-> (bits, metrics, the six counters of this call's list-of-32 launch)"""
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
        got = tuple(g.debug_get(k) for k in NAMES)
    finally:
        for k in knobs:
            g.debug_set(k, 0)
    return out.cpu().numpy(), pm.cpu().numpy(), got


def frozen_of(o):
    return np.asarray(o.frozen(), np.uint8)


def marks_of(o, g):
    """rb per leaf by the model's statement of the host rule; the uploaded words carry exactly that field and nothing above it."""
    fr = frozen_of(o)
    rb = r1_model.marks(fr, r1_model.weak_leaves(fr))
    assert ((g.debug_ctl_words(True) >> 9) == rb).all()
    return rb


def both_ways(o, g, llr, L, knobs=None, want=None, model=True):
    """model: True = the six counters must equal the CPU model's; False = inputs the model cannot follow (metric ties): the
    continuation must at least have committed something; None = no count is asserted. -> (oracle bits, counters)"""
    want = o.decode_scl_llr(llr, L) if want is None else want
    bits, pm, got = decode(g, llr, L, False, knobs)
    bits1, pm1, got1 = decode(g, llr, L, True, knobs)
    print(llr.shape, L, knobs, dict(zip(NAMES, got)))
    assert got1 == (0,) * 6                                 # no marks: no continuation ever starts
    assert got[3] <= got[2] and got[5] <= got[4]
    if model:
        assert got == r1_chain_model.six(r1_chain_model.counts(frozen_of(o), llr, L)), got
    if model is False or (model and llr.shape[0] >= 8):
        assert got[0] > 0, got
    assert (bits == want).all(), np.nonzero((bits != want).any(axis=1))[0][:10]
    assert (bits1 == want).all(), np.nonzero((bits1 != want).any(axis=1))[0][:10]
    assert (pm.view(np.uint64) == pm1.view(np.uint64)).all(), np.nonzero(pm != pm1)[0][:10]
    return want, got


# ---- the generic-N object: no tables, no head
@pytest.mark.parametrize("code", ((8, 128, 8), (9, 128, 8)), ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("tuning", (0, 16))
def test_generic_n(hooks_lib, oracle_built, code, tuning):
    o, g, llr = setup(code)
    assert g.debug_get("test_hooks") == 1
    rb = marks_of(o, g)
    assert (rb == 3).sum() > 0
    g.set_tuning(waves_per_cu=tuning)
    try:
        want, got = both_ways(o, g, llr, 32)
        assert min(got[2:]) > 0, got                       # both sequels tried and committed
        for B in (1, 2, 3):
            both_ways(o, g, llr[40 - B:], 32, want=want[40 - B:])
            both_ways(o, g, llr[:B], 32, want=want[:B])
    finally:
        g.set_tuning(waves_per_cu=0)


@pytest.mark.parametrize("L", (17, 24, 31))
def test_list_sizes_below_the_group(hooks_lib, oracle_built, L):
    """Lanes >= L are never active: a full list is nact == L, before and after a ranking step."""
    for code in ((8, 128, 8), (9, 128, 8)):
        o, g, llr = setup(code)
        _, got = both_ways(o, g, np.concatenate([llr[:7], llr[-8:]]), L)
        assert got[2] > 0 and got[4] > 0, got


def test_high_rate_block_before_the_list_is_full(hooks_lib, oracle_built):
    """(6, 48, 0): the first marked block starts at the sixth unfrozen leaf — just full. An explicit mask at N = 64 whose FIRST
    unfrozen leaves are the marked quad [28, 32): one path there, its first leaf takes the general path with a list that is not
    full, and the entry after a ranking step must not open."""
    o, g, llr = setup((6, 48, 0), B=21, snrs=(1.0, 6.0))
    marks_of(o, g)
    both_ways(o, g, llr, 32)
    both_ways(o, g, llr[:1], 32)
    o, g, llr = from_mask(("explicit", "early-quad"), 6, list(range(28, 32)) + list(range(40, 64)), 21)
    rb = marks_of(o, g)
    assert rb[28] == 2 and rb[40] == 3
    both_ways(o, g, llr, 32)
    rb0 = rb.copy()
    rb0[28] = 0
    assert r1_chain_model.counts(frozen_of(o), llr, 32, rb0) == r1_chain_model.counts(frozen_of(o), llr, 32, rb)


# ---- the fixed-N objects: table mode and the two-phase form (units 2 and 6)
HEAD_PHI = {(10, 512, 16): 0, (10, 256, 8): 368, (11, 1024, 16): 432}       # hand-over leaf of the two-phase form (0: one phase)


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
        marks_of(o, g)
        _, got = both_ways(o, g, llr, 32, knobs, want=want, model=False)
        assert got[3] > 0 and got[5] > 0, got
        assert g.debug_get("head_phi") == (HEAD_PHI[code] if form == "head" else 0)
        both_ways(o, g, llr[37:], 32, knobs, want=want[37:])          # (three rows: a wave with one valid codeword; counts = the model's)
    finally:
        g.set_tuning(waves_per_cu=0)


# ---- explicit masks (from_tables), N = 512, no CRC: unfrozen runs placed by hand (the first four: tests/test_gpu_r1_block.py)
def _run(a, b):
    return list(range(a, b))


EXPLICIT = {
    # 25 unfrozen leaves, then the octet [448, 456): its 7th leaf is the 32nd unfrozen step -> the octet and its second quad are
    # not marked, the first quad is: the chain must not run on the shrunk octet
    "flush-inside-octet": _run(423, 448) + _run(448, 456) + _run(480, 512),
    # 24 before: the octet's LAST leaf is the 32nd step -> marked; a chained octet is followed by the flush of the history word
    "flush-after-octet": _run(424, 448) + _run(448, 456) + _run(480, 512),
    # 28 before a quad whose last leaf is the 32nd step, and the mask ends in an octet at N - 1
    "flush-after-quad": _run(404, 432) + _run(432, 436) + _run(496, 512),
    # a quad and an octet in channels no construction would use (weak leaves: never marked) once the list is full
    "weak-block": _run(96, 104) + _run(128, 132) + _run(136, 144) + _run(448, 512),
    # eight unfrozen leaves fill the list, 24 frozen leaves follow, then the marked octet [448, 456): its leaf 0 is the first leaf of
    # a subtree of 64 behind a frozen run — the least reliable of the block, almost always ranked; then entry after the ranking step
    # and the chain in one step
    "ranked-octet": _run(416, 424) + _run(448, 456) + _run(480, 512),
}


@pytest.mark.parametrize("name", sorted(EXPLICIT))
def test_explicit_masks(hooks_lib, oracle_built, name):
    o, g, llr = from_mask(("explicit", name), 9, EXPLICIT[name], 24)
    rb = marks_of(o, g)
    if name == "flush-inside-octet":
        assert rb[448] == 2 and rb[452] == 0
    if name in ("flush-after-octet", "ranked-octet"):
        assert rb[448] == 3 and rb[452] == 2
    want, got = both_ways(o, g, llr, 32)
    both_ways(o, g, llr[:3], 32, want=want[:3])
    if name == "ranked-octet":
        assert got[3] > 0 and got[5] > 0, got
        # (what the mask is for, by the model the counters were just found equal to: octets finished in one step after a ranked
        # first leaf. Leaf 448 itself is ranked in every wave; its own continuation rarely passes — the leaves behind it are
        # weak as well —, the octets of the run [480, 512) supply the commits)
        assert r1_chain_model.counts(frozen_of(o), llr, 32)["rank_then_chain"] > 0
    assert len({tuple(r[:16]) for r in want}) > 1


# ---- values
@pytest.mark.parametrize("scale", (30.0, 300.0))
def test_l_form_values_and_underflowing_products(hooks_lib, oracle_built, scale):
    """Rows scaled so that |x| >= 690 (L-form) and g products below e^-690 occur inside the blocks. The saturated metrics tie, so
    the CPU model cannot follow these rows. x 30: the continuation must have run (committed > 0). x 300: no leaf step is fast, every
    marked quad is entered after a ranking step — good and bad forks tie, the tests give it up; no count is asserted there."""
    o, g, llr = setup((9, 128, 8))
    both_ways(o, g, llr[10:31] * scale, 32, model=False if scale == 30.0 else None)


def test_exact_zero_leaf_llrs(hooks_lib, oracle_built):
    """Rows of +-1 and +-3 with the signs of noisy codewords: g-nodes whose operands cancel give LLR 0 exactly — a stored value of
    magnitude 1.0, which decides 0 whatever its sign bit: the give-ups over |v| == 1.0 on the new entries. Every metric of such a
    row ties, so the CPU model cannot follow it and no count is asserted; bits against the oracle, bits and metrics against no_r1."""
    o, g, llr = setup((9, 128, 8))
    sg = np.where(llr[:20] < 0, -1.0, 1.0)
    both_ways(o, g, np.concatenate([sg[:10], 3.0 * sg[10:]]), 32, model=None)
