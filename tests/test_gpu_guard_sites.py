"""GPU suite: the fallback set for windows BELOW g-branches. tests/test_gpu_fallback_rows.py plants its windows on layers 1 and 2 of
the first descent, which every path shares and which a handful of the guard-carrying source sites serve. Here the window sits at
an f-node that a path reaches only after deciding: guard_numpy.plant_node rewrites the channel block under one node so that the
reference's own arithmetic delivers |x| = 40 + delta at one element of its input (exactly: min-sum copies through the f-steps,
exact halves through the g-steps), at the sites of guard_numpy.node_sites —

    hbm    after f, g (phi = N / 4): layer 3, the f-stage of the fused pass that starts with a g-visit; HBM-scratch rows
    table  after g (phi = N / 2): layer 2 — the first f-stage of the four-layer pass, or in table mode the table build (kind 2)
    gf     after g, f: layer 3 — the second f-stage of the four-layer pass (in table mode: fed from the table)
    gff    after g, f, f: layer 4 — its third f-stage
    mid    a node with an input of 32 elements: HBM-scratch rows in, out
    lds    a node with an input of 8 elements: LDS layers (list size 1, one codeword per wave: the mixed node of 8 in registers)
    regs   a node with an input of 4 elements: registers in the one-codeword-per-wave list kernel
    late   the last mixed node of the codeword, beyond 3 N / 4: the per-lane guard distance is kept to the codeword's end, also
           behind the two-phase head

— and, in table mode, in a HYPOTHESIS of the table build that no living path holds (flagged there, not flagged where the paths
visit layer 2 themselves). As in the other file: the fallback set is EXACTLY the rows planted inside the window, every row's bits
are the oracle's, and the kernel that the variant means ran. tests/test_guard_model.py proves on the CPU that each planted f-node
is evaluated for a living path at |delta| exactly and that every other evaluated f-node of every row, planted or ordinary, is more
than 1e-3 away. Device-pointer entry points only.

The 32- and 16-bit formats hold no |x| = 40 + delta but delta = 0: their batches (list size 1) carry inside plants only."""
import numpy as np
import pytest

import guard_numpy as G
from scl_list_numpy import Code
from test_gpu_fallback_rows import ED_VARIANTS, LARGE, LARGE_VARIANTS, MID, _case, _decode, _forced

pytestmark = pytest.mark.gpu

_codes = {}


def _code(key):
    if key not in _codes:
        _codes[key] = Code(_case(key).o)
    return _codes[key]


def _check(key, L, knobs, lat, head=False, fmt="f64", tables=True, hyp=False, b=None):
    """Every node batch of the code and format (hyp: the hypothesis batch alone) through one family and variant."""
    c, code = _case(key), _code(key)
    b = c.base.shape[0] if b is None else b
    names = tuple(s for s in G.SITE_NAMES if s != "regs") if key == LARGE else G.SITE_NAMES
    batches = [G.hypothesis_batch(code)] if hyp else G.node_batches(code, fmt, names=names)
    for k, batch in enumerate(batches):
        rows, expect = G.planted(c.base[:b], batch, L, fmt, tables=tables)
        want = c.want(rows, fmt, L, b, ("nodes", hyp, k))
        with _forced(c, knobs):
            bits, fb = _decode(c, rows, fmt, L)
            waves, phi = c.g.debug_get("lat_waves"), c.g.debug_get("head_phi")
        assert (waves > 0) == lat and (phi > 0) == head, (waves, phi)
        assert "lat_grid" not in knobs or waves == knobs["lat_grid"]
        print(f"{key} L={L} {fmt} {knobs} batch {k}: fallback set {None if fb is None else fb.tolist()}, planted {expect.tolist()}")
        assert fb is not None and fb.dtype == np.uint32 and np.array_equal(fb, expect), \
            (k, batch, None if fb is None else fb.tolist(), expect.tolist())
        bad = np.nonzero((bits != want).any(axis=1))[0]
        assert bad.size == 0, f"rows {bad.tolist()} of batch {k} differ from the oracle"


# ---- list size 1 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["f64", "f32", "f16", "bf16"])
@pytest.mark.parametrize("fold", [0, 1])
def test_sc8(built_lib, oracle_built, fold, fmt):
    """sc8_decode_kernel: the plain visits, the three stages of the folded chains (after a g-visit and at a left descent), the
    visits of 4, 2 and 1 elements; with the folded top and with the conversion pass."""
    _check(MID, 1, {"lat_max_b": -1, "sc_no_fold": 1 - fold}, lat=False, fmt=fmt)


def test_sc_lat(built_lib, oracle_built):
    """sc_lat_kernel: visits of 64 elements and more, of fewer, and the mixed node of 8 decoded in registers."""
    _check(MID, 1, {}, lat=True)


# ---- the lists ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [2, 4, 8])
def test_list_lat(built_lib, oracle_built, L):
    """The one-codeword-per-wave form: stored layers, and the two lowest layers on registers."""
    _check(MID, L, {}, lat=True)


@pytest.mark.parametrize("L", [2, 4, 8])
def test_list_lat_one_wave_decodes_ordinary_rows_after_planted_ones(built_lib, oracle_built, L):
    """ONE wave takes 14 rows in order: rows 1, 2 and 6 .. 12 are ordinary ones decoded right after a planted one, in the LDS the
    planted row left behind. The lanes of a path that is not active run the layer visits on whatever their slots hold — early in a
    codeword the previous codeword's values, the planted pair among them — and what they evaluate must not count: the ordinary
    rows stay out of the fallback set. (With the work of 70 rows spread over many waves the order is not fixed, and a kernel
    that counted it flagged an ordinary row in one run and not in the next.)"""
    _check(MID, L, {"lat_grid": 1}, lat=True, b=14)


@pytest.mark.parametrize("variant", list(ED_VARIANTS))
@pytest.mark.parametrize("L", [4, 8, 16, 32])
def test_batch_ed(built_lib, oracle_built, L, variant):
    """The batch kernel: fused two- and four-layer passes, the LDS bottom of the tree, the generic visit (all of the register-double-
    buffered geometry)."""
    _check(MID, L, dict(ED_VARIANTS[variant], lat_max_b=-1), lat=False)


@pytest.mark.parametrize("variant", list(LARGE_VARIANTS))
def test_batch_ed_large_code(built_lib, oracle_built, variant):
    """N = 2048, list of 32: every site under the small-batch geometry, table mode and its absence, the two-phase head (the late
    site lies behind the hand-over) and its absence."""
    knobs, head = LARGE_VARIANTS[variant]
    _check(LARGE, 32, knobs, lat=False, head=head)


@pytest.mark.parametrize("variant,tables", [("tables", True), ("no_tables", False)])
def test_table_build_flags_hypotheses_no_path_holds(built_lib, oracle_built, variant, tables):
    """The table build at phi = N / 2 evaluates the layer-2 f-nodes under all four pairs of partial-sum bits: a window that only a
    pair no path holds meets is flagged in table mode and is not where the paths visit layer 2 themselves; the living-path plant
    of the same batch is flagged in both."""
    knobs, head = LARGE_VARIANTS[variant]
    _check(LARGE, 32, knobs, lat=False, head=head, tables=tables, hyp=True)


def test_r1_blocks(built_lib, oracle_built):
    """The f-nodes inside the rate-1 quad and octet continuations of the list of 32 (guard_numpy.R1_PLANTS), on the product
    library; tests/test_gpu_guard_r1.py runs the same rows on the test library, whose counters show that the planted blocks were
    finished in one step."""
    c, code = _case(MID), _code(MID)
    rows, expect, _, _ = G.r1_batch(code, c.base)
    want = c.o.decode_scl_llr(rows, G.R1_L)
    with _forced(c, {"lat_max_b": -1}):
        bits, fb = _decode(c, rows, "f64", G.R1_L)
        assert c.g.debug_get("lat_waves") == 0
    print(f"rate-1 blocks: fallback set {None if fb is None else fb.tolist()}, planted {expect.tolist()}")
    assert fb is not None and fb.dtype == np.uint32 and np.array_equal(fb, expect), (None if fb is None else fb.tolist(), expect.tolist())
    assert (bits == want).all(), np.nonzero((bits != want).any(axis=1))[0]


# ---- the weak-leaf guard ----------------------------------------------------------------------------------------------------------------

class _WeakCase:
    """The code of guard_numpy.WEAK_CODE: oracle, handle (it reports weak leaves), the rows with the plants applied (the list
    sizes above 1 all get the same rows) and the oracle's bits per list size."""

    def __init__(self):
        import ctypes as C
        import polar_amd
        from oracle_lib import Oracle
        n, K, eps, crc = G.WEAK_CODE
        self.N, self.K = 1 << n, K
        self.o = Oracle(n, K, eps, crc, srand=1)
        C.CDLL(None).srand(C.c_uint(1))
        self.g = polar_amd.PolarCode(n, K, eps, crc)
        code = Code(self.o)
        # (the model's weak leaves are the library's: bit 8 of the uploaded control words, which the kernel's guard reads)
        assert self.g.weak_leaves == int(G.weak_mask(code).sum()) > 0
        assert np.array_equal((self.g.debug_ctl_words(False) >> 8) & 1, G.weak_mask(code))
        self.batch = G.weak_batch(code)
        self.rows, planted = G.planted(G.weak_rows(self.o), self.batch, 4)
        self.expect = np.array(sorted(set(planted.tolist()) | set(G.WEAK_FLAGGED)), np.uint32)
        self._want = {}

    def want(self, L):
        if L not in self._want:
            self._want[L] = self.o.decode_scl_llr(self.rows, L)
        return self._want[L]


_weak = []


@pytest.mark.parametrize("family,L,knobs,lat", [("ListLat", 4, {}, True), ("BatchEd", 8, {"lat_max_b": -1}, False),
                                                ("BatchEd", 32, {"lat_max_b": -1}, False)])
def test_weak_leaf_guard(built_lib, oracle_built, family, L, knobs, lat):
    """A weak unfrozen leaf within 1e-8 of a tie hands the codeword to the fallback pass: the planted leaf LLRs 5e-9 and 0.99e-8
    are flagged, 1.01e-8 and 2e-8 are not, and of the ordinary rows exactly those that the model flags (guard_numpy.WEAK_FLAGGED;
    the rows of WEAK_LEFT_OUT, too close to call by the model, may fall on either side). Every row's bits are the oracle's."""
    if not _weak:
        _weak.append(_WeakCase())
    c = _weak[0]
    assert L in G.WEAK_LS
    with _forced(c, knobs):
        bits, fb = _decode(c, c.rows, "f64", L)
        waves = c.g.debug_get("lat_waves")
    assert (waves > 0) == lat, waves
    print(f"weak leaves, {family} L={L}: fallback set {None if fb is None else fb.tolist()}, expected {c.expect.tolist()}")
    assert fb is not None and fb.dtype == np.uint32
    keep = ~np.isin(fb, G.WEAK_LEFT_OUT)
    assert np.array_equal(fb[keep], c.expect), (fb.tolist(), c.expect.tolist())
    bad = np.nonzero((bits != c.want(L)).any(axis=1))[0]
    assert bad.size == 0, f"rows {bad.tolist()} differ from the oracle"
