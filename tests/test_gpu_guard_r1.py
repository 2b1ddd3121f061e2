"""GPU suite: the fallback set for windows INSIDE the rate-1 quad and octet continuations of the list of 32
(polar_amd/csrc/polar_scl_leaf.inc). A marked block of four unfrozen leaves is finished in the step of its first leaf, the second
quad of a marked octet in the same step; the f-nodes evaluated in there add their guard distance to a temporary that reaches the
lane's own only when the block is committed. A lost write-back computes the same bits: only a row whose window sits at one of those
f-nodes, in a block that really is committed in one step, shows it.

guard_numpy.R1_PLANTS puts such a window at each of the five f-node calls of the continuation (the last f-node of the first quad —
in a quad outside any octet, so that no chained quad carries its distance along —, the two f-nodes on the second quad's input, the
one of its first leaf and its last), each with a control just outside the window as the other codeword of its wave.
tests/test_guard_model.py proves on the CPU that the plants sit there and nowhere else and that the model of
tests/r1_chain_model.py finishes every planted block in one step. Here, on the TEST build of the library, whose list-of-32 units
count the continuations of a launch: the fallback set is exactly the rows planted inside, every row's bits are the oracle's, and
the six counters equal the model's — for the batch and for every planted wave alone. Under "no_r1" (control words without the
marks: every leaf a loop step) the counters are zero and the same rows are flagged through the loop's own f-nodes."""
import ctypes as C

import numpy as np
import pytest

import guard_numpy as G
import r1_chain_model
from scl_list_numpy import Code
from test_gpu_fallback_rows import MID, _decode, _forced

pytestmark = pytest.mark.gpu

NAMES = ("r1_committed", "r1_discarded", "r1_rank_tried", "r1_rank_committed", "r1_chain_tried", "r1_chain_committed")
_cache = {}


class _Case:
    """The MID code on the library in use when it is first asked for (a handle of its own: the test build), the planted rows, the
    oracle's bits and the model's leaf tests per row."""

    def __init__(self):
        import polar_amd
        from oracle_lib import Oracle
        n, K, crc = MID
        self.K = K
        self.o = Oracle(n, K, G.EPS, crc, srand=1)
        C.CDLL(None).srand(C.c_uint(1))
        self.g = polar_amd.PolarCode(n, K, G.EPS, crc)
        assert self.g.debug_get("test_hooks") == 1 and self.g.weak_leaves == 0
        self.code = Code(self.o)
        self.rows, self.expect, self.blocks, _ = G.r1_batch(self.code, G.base_rows(self.o, MID))
        self.want = self.o.decode_scl_llr(self.rows, G.R1_L)
        self.frozen = np.asarray(self.code.frozen, np.uint8)
        self.tests, self.done = [], {}
        for w in range(0, G.R1_B, 2):
            self.done[w], t = G.r1_wave(self.code, self.rows[w:w + 2])
            self.tests += t

    def model(self, lo, hi):
        return r1_chain_model.six(r1_chain_model.counts(self.frozen, self.rows[lo:hi], G.R1_L, tests=self.tests[lo:hi]))


def _case():
    if not _cache:
        _cache[0] = _Case()
    return _cache[0]


def _run(c, lo, hi, no_r1):
    """Rows lo .. hi - 1 through the batch kernel -> (bits, fallback set, the six counters of the launch)."""
    with _forced(c, {"lat_max_b": -1}):
        c.g.debug_set("no_r1", 1 if no_r1 else 0)
        try:
            bits, fb = _decode(c, c.rows[lo:hi], "f64", G.R1_L)
            got = tuple(c.g.debug_get(k) for k in NAMES)
            assert c.g.debug_get("lat_waves") == 0
        finally:
            c.g.debug_set("no_r1", 0)
    assert fb is not None and fb.dtype == np.uint32
    bad = np.nonzero((bits != c.want[lo:hi]).any(axis=1))[0]
    assert bad.size == 0, f"rows {(bad + lo).tolist()} differ from the oracle"
    return fb, got


def test_planted_blocks_are_committed_in_one_step_and_flagged(hooks_lib, oracle_built):
    c = _case()
    fb, got = _run(c, 0, G.R1_B, False)
    print(f"rate-1 blocks: fallback set {fb.tolist()}, planted {c.expect.tolist()}, counters {dict(zip(NAMES, got))}")
    assert got == c.model(0, G.R1_B), (got, c.model(0, G.R1_B))
    assert np.array_equal(fb, c.expect), (fb.tolist(), c.expect.tolist())
    for w, phi0, kind in c.blocks:
        assert (phi0, kind) in c.done[w]                                    # (the model finishes the planted block in one step ...)
        fb, got = _run(c, w, w + 2, False)
        print(f"wave of rows {w}, {w + 1}: block at leaf {phi0} ({kind}), fallback set {fb.tolist()}, counters {dict(zip(NAMES, got))}")
        assert got == c.model(w, w + 2), (w, got, c.model(w, w + 2))        # (... and the wave alone does what the model says)
        assert got[0] > 0 and (kind == "quad" or got[5] > 0), (w, got)
        assert np.array_equal(fb + w, c.expect[(c.expect >= w) & (c.expect < w + 2)]), (w, fb.tolist())


def test_the_same_rows_are_flagged_through_the_loop(hooks_lib, oracle_built):
    c = _case()
    fb, got = _run(c, 0, G.R1_B, True)
    print(f"rate-1 blocks, no_r1: fallback set {fb.tolist()}, planted {c.expect.tolist()}")
    assert got == (0,) * 6, got
    assert np.array_equal(fb, c.expect), (fb.tolist(), c.expect.tolist())
