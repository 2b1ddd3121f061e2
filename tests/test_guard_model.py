"""CPU suite: the conditions on the inputs that tests/test_gpu_fallback_rows.py rests on, proven on the oracle and numpy alone, so
that the model of tests/guard_numpy.py — and not what a kernel happens to flag — decides which rows are expected in the fallback
set. If a row breaks a condition here, choose another seed or block in guard_numpy's table; the GPU assertions are not widened.

The nodes BELOW the first descent of a list decode depend on the paths' decisions: guard_numpy.list_margins walks the list as the
reference does and the second half of this file proves the same for them — the ordinary rows keep 1e-3 at every f-node evaluated
for a living path at every list size the GPU tests use, and the plants of tests/test_gpu_guard_sites.py sit where they are meant
to sit and nowhere else."""
import math

import numpy as np
import pytest

import guard_numpy as G
from scl_list_numpy import Code, split

FMTS = ("f64", "f32", "f16", "bf16")
_cache = {}


def _case(key):
    """(oracle, Code, base rows [B][N]) of a code of the table; the rows are never changed."""
    if key not in _cache:
        from oracle_lib import Oracle
        n, K, crc = key
        o = Oracle(n, K, G.EPS, crc, srand=1)
        _cache[key] = (o, Code(o), G.base_rows(o, key))
    return _cache[key]


def test_deltas_against_both_window_forms():
    """E = exp(-(40 + delta)) on the host against the two window forms of DESIGN.md (the constants are restated in guard_numpy, not
    imported from the kernels' header): 0 and +-5e-11 lie inside both, +-1e-9 outside both; -2e-10 is inside the per-lane form only
    (the documented superset), which is why no plant uses it."""
    for d in G.DELTAS_IN:
        E = math.exp(-(40.0 + d))
        assert G.in_wave_window(E) and G.in_lane_window(E), d
    for d in G.DELTAS_OUT:
        E = math.exp(-(40.0 + d))
        assert not G.in_wave_window(E) and not G.in_lane_window(E), d
    E = math.exp(-(40.0 - 2e-10))
    assert not G.in_wave_window(E) and G.in_lane_window(E)
    # (the kernels' own exp is good to a few 1e-16 relative: 5e-11 from either edge is 1e5 times that)
    assert abs(math.exp(-40.0) / G.E40 - 1) < 1e-15


def test_input_guard_is_applied_to_the_widened_value():
    assert G.input_guard(np.array([1.0, np.float32(1e-9)], np.float32)) and float(np.float32(1e-9)) < 1e-9
    assert not G.input_guard(np.array([1.0, 1e-9])) and not G.input_guard(np.array([1.0, -1.0000001e-9]))
    assert G.input_guard(np.array([1.0, 9.99e-10])) and G.input_guard(np.array([0.0, 1.0])) and G.input_guard(np.array([1.0, -0.0]))
    assert G.input_guard(np.array([1.0, np.inf])) and G.input_guard(np.array([-np.inf, 1.0])) and G.input_guard(np.array([np.nan, 1.0]))
    assert not G.input_guard(np.array([2.0 ** -24, 1.0], np.float16)) and G.input_guard(np.array([0x0000, 0x3F80], np.uint16))
    assert G.row_tiny(np.array([0.09, -0.0999])) and not G.row_tiny(np.array([0.09, -0.1]))


@pytest.mark.parametrize("key", list(G.CODES))
def test_codes_and_ordinary_rows(built_lib, oracle_built, key):
    """No weak leaf; a frozen prefix shorter than N / 2 (so every family evaluates layer 2 of the first descent); no ordinary row is
    flagged by a criterion on the input in any element format, and none comes within 1 of |x| = 40 on its first descent."""
    import polar_amd
    o, code, llr = _case(key)
    n, K, crc = key
    g = polar_amd.PolarCode(n, K, G.EPS, crc)
    assert g.weak_leaves == 0
    g.close()
    prefix = int(np.argmin(code.frozen)) if not code.frozen.all() else code.N
    assert code.frozen[:prefix].all() and prefix < code.N // 2
    for fmt in FMTS:
        rows = G.narrow(llr, fmt)
        for r in range(rows.shape[0]):
            assert not G.input_guard(rows[r]) and not G.row_tiny(rows[r]), (fmt, r)
    for r in range(llr.shape[0]):
        assert G.first_descent(llr[r]).min() > 1, r


@pytest.mark.parametrize("key", list(G.CODES))
def test_plants_do_what_their_class_says(oracle_built, key):
    """Every plant of every batch and format, on the criteria on the input: window plants sit |delta| from 40 at their layer (to
    1e-13) and more than 1 away at every other; input plants trip input_guard and nothing else does; the tiny row is row_tiny and its
    control, at a largest magnitude of exactly 0.1, is neither that nor below 1e-9 anywhere."""
    o, code, llr = _case(key)
    N = code.N
    for fmt in FMTS:
        for batch in G.batches(N, fmt):
            rows, want = G.planted(llr, batch, 4, fmt)
            pos = G.planted_positions(rows.shape[0])
            assert want.tolist() == [r for r, pl in zip(pos, batch) if pl.flag_list]
            for r in range(rows.shape[0]):
                if r not in pos:
                    assert np.array_equal(rows[r], G.narrow(llr[r], fmt))
            for r, pl in zip(pos, batch):
                row = rows[r]
                assert G.input_guard(row) == (pl.kind == "input"), (fmt, pl)
                assert G.row_tiny(row) == (pl.kind == "tiny"), (fmt, pl)
                d = G.first_descent(row)
                if hasattr(pl, "site"):
                    layer = pl.site[0]
                    assert abs(d[layer - 1] - abs(pl.delta)) < 1e-13, (pl, d[layer - 1])
                    assert np.delete(d, layer - 1).min() > 1, (pl, d)
                    assert (abs(pl.delta) < 1e-10) == pl.flag_list
                elif pl.kind in ("control", "tiny") and np.isfinite(G.widen(row)).all():
                    assert d.min() > 1, (pl, d)
                if pl.name == "largest magnitude 0.1":
                    a = np.abs(G.widen(row))
                    assert a.max() == np.abs(G.widen(G.narrow(np.array([0.1]), fmt)))[0] >= 0.1 and a.min() > 1e-9


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("key", [k for k in G.CODES if k[0] <= 9])
def test_list_size_1_margins(oracle_built, key, fmt):
    """The list-size-1 kernels have criteria of their own below the channel: a product bound (1e-8) and a zero root at all-unfrozen
    nodes, a sum bound (690) at all-frozen ones, and the window at EVERY f-node of the pass. Along the oracle's decisions, every
    ordinary row and every planted row that the input guard does not flag anyway stays a factor of 100 away from the first two, has
    no zero root, and comes within 1e-3 of the window at the planted node only. In every element format the GPU test feeds these kernels
    (the rows as widened)."""
    o, code, llr = _case(key)

    def check(row, plant):
        row = G.widen(row)
        u = G.sc_decisions(code, row)
        assert np.array_equal(split(code, u)[0], o.decode_scl_llr(row, 1)), plant          # (the oracle's decisions)
        prod, fsum, zero, win = G.l1_margins(code, row, u)
        assert prod >= 1e-6 and fsum <= 600 and not zero, (plant, prod, fsum, zero)
        near = np.sort(win[win < 1e-3])
        if plant is not None and hasattr(plant, "site"):
            assert near.size == 1 and abs(near[0] - abs(plant.delta)) < 1e-13, (plant, near)
        else:
            assert near.size == 0, (plant, near)

    plain = G.narrow(llr, fmt)
    for r in range(llr.shape[0]):
        check(plain[r], None)
    for batch in G.batches(code.N, fmt):
        rows, _ = G.planted(llr, batch, 1, fmt)
        for r, pl in zip(G.planted_positions(rows.shape[0]), batch):
            if pl.flagged(1) is not None and pl.kind != "input":
                check(rows[r], pl)


# ---- below the first descent: the list walk (tests/test_gpu_guard_sites.py rests on these) ------------------------------------------

SMALL, MID, LARGE = (7, 64, 8), (9, 256, 8), (11, 1024, 16)
LIST_SIZES = {SMALL: (2, 4, 8), MID: (2, 4, 8, 16, 32), LARGE: (32,)}       # every list size a GPU test decodes that code's rows at


def _site_names(key):
    return tuple(s for s in G.SITE_NAMES if s != "regs") if key == LARGE else G.SITE_NAMES


def test_weak_mask_and_pruned_nodes(oracle_built):
    """The codes of the table have no weak leaf by the restated recursion either (derive_tables counts the same: test_codes_and_
    ordinary_rows); a code of the fuzz test's kind has. The pruned pass computes the root's input and the inputs of the children of
    mixed nodes only."""
    from oracle_lib import Oracle
    for key in G.CODES:
        assert not G.weak_mask(_case(key)[1]).any()
    code = Code(Oracle(9, 505, 0.7, 0, srand=1))
    weak = G.weak_mask(code)
    assert weak.any() and not (weak & (code.frozen != 0)).any()
    code = _case(SMALL)[1]
    nodes = G.pruned_nodes(code)
    assert (0, 0) in nodes
    for d, i in nodes:
        if d:
            fz = code.frozen[(i >> 1) * (code.N >> (d - 1)):((i >> 1) + 1) * (code.N >> (d - 1))]
            assert fz.any() and not fz.all()


@pytest.mark.parametrize("key", list(G.CODES))
def test_sites_are_evaluated_by_every_family(oracle_built, key):
    """Every site is an f-node on the input of a MIXED node with a mixed left child, below at least one g-branch: the pruned
    list-size-1 pass computes its output, and so does a list kernel (the output feeds an unfrozen leaf, and is no inner node of an
    all-frozen block of 4 or 8 leaves). The late site starts beyond 3 N / 4."""
    code = _case(key)[1]
    nodes = G.pruned_nodes(code)
    for name, (path, j) in G.node_sites(code).items():
        d, i = len(path), G.node_index(path)
        assert sum(path) >= 1 and (d + 1, 2 * i) in nodes and (d + 2, 4 * i) in nodes, (name, path)
        assert not code.frozen[i * (code.N >> d):(2 * i + 1) * (code.N >> (d + 1))].all()
    path = G.node_sites(code)["late"][0]
    assert G.node_index(path) * (code.N >> len(path)) >= 3 * code.N // 4


@pytest.mark.parametrize("key", list(G.CODES))
def test_ordinary_rows_keep_their_distance_at_every_node_of_a_list_decode(oracle_built, key):
    """Every ordinary row, at every list size a GPU test decodes it at: no f-node evaluated for a living path — nor, on the large
    code, for a hypothesis of the table build — within 1e-3 of |x| = 40, no tie, the model's winner is the oracle's. And the
    SKIPPED trials are skipped for that reason and no other."""
    o, code, llr = _case(key)
    for L in LIST_SIZES[key]:
        want = o.decode_scl_llr(llr, L)
        for r in range(llr.shape[0]):
            m = G.list_margins(code, llr[r], L, tables=(key == LARGE))
            assert m.near(1e-3) == [], (L, r, m.near(1e-3))
            assert np.array_equal(m.info, want[r]), (L, r)
    for t in G.SKIPPED[key]:
        row = o.synth_llr_trials(G.CODES[key], [t], o.snr_sqrt_linear(G.EBNO))[0][0]
        assert any(G.list_margins(code, row, L, tables=(key == LARGE)).near(1e-3) for L in LIST_SIZES[key]), t


def _check_node_plant(o, code, row, pl, L, both):
    """One planted row at one list size (both: under both values of `tables`)."""
    assert not G.input_guard(row) and not G.row_tiny(row), pl
    path, j = pl.node
    d = len(path)
    at = (d + 1, j, G.node_index(path) * (code.N >> d))
    for tables in ((False, True) if both else (False,)):
        m = G.list_margins(code, row, L, tables)                               # (raises TieError on a tie)
        near = m.near(1e-3)
        assert all(abs(x[0] - abs(pl.delta)) < 1e-13 for x in near), (pl, L, tables, near)
        living = [x[1:] for x in near if x[3] >= 0]
        hyps = [x[1:3] for x in near if x[3] < 0]
        if pl.flag_l1 is None:                                                 # in a hypothesis that no path holds, and only there
            assert living == [] and bool(hyps) == tables and all(h == (2, j) for h in hyps), (pl, L, tables, near)
        else:
            assert living == [at] and all(h == at[:2] for h in hyps), (pl, L, tables, near, at)
        assert np.array_equal(m.info, o.decode_scl_llr(row[None], L)[0]), (pl, L)


@pytest.mark.parametrize("key", [MID, LARGE])
def test_node_plants_sit_where_they_are_meant_to(oracle_built, key):
    """Every plant of tests/test_gpu_guard_sites.py at every list size it is decoded at: the planted f-node is evaluated for a living
    path (a hypothesis plant: for a hypothesis only, under tables=True only) at exactly |delta| (to 1e-13), every other evaluated
    f-node, under both values of `tables`, is more than 1e-3 away, no tie, no input criterion, the winner is the oracle's."""
    o, code, llr = _case(key)
    batches = G.node_batches(code, names=_site_names(key))
    if key == LARGE:
        batches.append(G.hypothesis_batch(code))
    for L in LIST_SIZES[key]:
        for batch in batches:
            rows, want = G.planted(llr, batch, L)
            pos = G.planted_positions(rows.shape[0])
            assert want.tolist() == [r for r, pl in zip(pos, batch) if pl.flag_list]
            for r, pl in zip(pos, batch):
                assert (abs(pl.delta) < 1e-10) == pl.flag_list
                _check_node_plant(o, code, rows[r], pl, L, key == LARGE)


@pytest.mark.parametrize("fmt", FMTS)
def test_node_plants_at_list_size_1(oracle_built, fmt):
    """The same plants along the single path of the list-size-1 kernels, in every element format they are fed in: the product, sum
    and zero-root criteria stay away, the window is met at the planted node alone, at |delta| exactly (a plant that the format
    moved would not be), the decisions are the oracle's."""
    o, code, llr = _case(MID)
    for batch in G.node_batches(code, fmt):
        rows, _ = G.planted(llr, batch, 1, fmt)
        for r, pl in zip(G.planted_positions(rows.shape[0]), batch):
            row = G.widen(rows[r])
            assert not G.input_guard(rows[r])
            u = G.sc_decisions(code, row)
            assert np.array_equal(split(code, u)[0], o.decode_scl_llr(row, 1)), pl
            prod, fsum, zero, win = G.l1_margins(code, row, u)
            assert prod >= 1e-6 and fsum <= 600 and not zero, (pl, prod, fsum, zero)
            near = win[win < 1e-3]
            assert near.size == 1 and abs(near[0] - abs(pl.delta)) < 1e-13, (fmt, pl, near)


def test_r1_block_plants_are_finished_in_one_step(oracle_built):
    """The plants inside the rate-1 quads and octets of the list of 32 (guard_numpy.R1_PLANTS): each sits at its f-node for a living
    path at exactly |delta| and nowhere else (no tie, no input criterion, the winner is the oracle's), every wave that holds one
    finishes the planted block in one step by the model of tests/r1_chain_model.py — the quad plant's block is a marked quad OUTSIDE
    any marked octet, so that no chained second quad carries its distance to the end; the chain plants' blocks are marked octets
    whose second quad is finished in the step of the first —, the plants cover the five f-node calls of the continuation, and the
    rows without a plant are the base rows."""
    import r1_model
    o, code, llr = _case(MID)
    rows, expect, blocks, pls = G.r1_batch(code, llr)
    assert rows.shape[0] == G.R1_B and set(G.planted_positions(G.R1_B)) <= set(pls)
    assert expect.tolist() == sorted(r for r, pl in pls.items() if pl.flag_list) and len(expect) == len(pls) // 2
    fr = np.asarray(code.frozen, np.uint8)
    rb = r1_model.marks(fr, r1_model.weak_leaves(fr))
    for r in range(G.R1_B):
        if r not in pls:
            assert np.array_equal(rows[r], llr[r])
            assert r ^ 1 not in pls
        else:
            assert (abs(pls[r].delta) < 1e-10) == pls[r].flag_list and pls[r ^ 1].block == pls[r].block
            _check_node_plant(o, code, rows[r], pls[r], G.R1_L, False)
    kinds = {(p[1], p[3]) for p in G.R1_PLANTS}
    assert kinds == {("quad", 0), ("chain_w", 0), ("chain_w", 1), ("chain_y", 0), ("chain_z", 0)}
    assert {p[5] for p in G.R1_PLANTS} == {1.0, -1.0} and {p[4] for p in G.R1_PLANTS} == set(G.DELTAS_IN + G.DELTAS_OUT)
    for w, phi0, kind in blocks:
        done, _ = G.r1_wave(code, rows[w:w + 2])
        assert (phi0, kind) in done, (w, phi0, kind, sorted(done))
        if kind == "quad":
            assert rb[phi0] == 2 and not (phi0 % 8 == 4 and rb[phi0 - 4] == 3) and (phi0, "chain") not in done
        else:
            assert rb[phi0] == 3 and phi0 % 8 == 0


def test_weak_mask_counts_the_librarys_weak_leaves(built_lib, oracle_built):
    """The restated recursion against derive_tables' own count, on the code of the weak-leaf tests."""
    import polar_amd
    import ctypes as C
    n, K, eps, crc = G.WEAK_CODE
    code = _weak_case()[1]
    C.CDLL(None).srand(C.c_uint(1))
    g = polar_amd.PolarCode(n, K, eps, crc)
    assert g.weak_leaves == int(G.weak_mask(code).sum()) > 0
    g.close()


# ---- the weak-leaf guard ----------------------------------------------------------------------------------------------------------------

def _weak_case():
    if "weak" not in _cache:
        from oracle_lib import Oracle
        n, K, eps, crc = G.WEAK_CODE
        o = Oracle(n, K, eps, crc, srand=1)
        _cache["weak"] = (o, Code(o), G.weak_rows(o))
    return _cache["weak"]


def test_weak_leaf_rows_and_plants(oracle_built):
    """The batch of the weak-leaf tests, by the model alone, at every list size used: the ordinary rows the model flags are the
    recorded ones, at least five ordinary rows fall on each side, at most 5 % are left out (smallest weak leaf in [0.9e-8, 1.1e-8],
    or an f-node within 1e-3 of the window); the planted rows deliver exactly the planted magnitude as their smallest weak leaf,
    keep 1e-3 from every window and no channel element below 1e-9; no row is tiny, no tie, every winner is the oracle's."""
    o, code, llr = _weak_case()
    assert G.weak_mask(code).sum() > 0 and G.weak_mask(code)[0]
    batch = G.weak_batch(code)
    pos = G.planted_positions(llr.shape[0])
    for L in G.WEAK_LS:
        rows, expect = G.planted(llr, batch, L)
        want = o.decode_scl_llr(rows, L)
        flagged, left_out, clear = [], [], []
        for r in range(rows.shape[0]):
            assert not G.input_guard(rows[r]) and not G.row_tiny(rows[r]) and np.abs(rows[r]).min() >= 1e-9, r
            m = G.list_margins(code, rows[r], L)
            assert np.array_equal(m.info, want[r]), (L, r)
            w = m.min_weak()
            if r in pos:
                pl = batch[pos.index(r)]
                assert w == abs(pl.value) == abs(m_leaf(m, pl.leaf)) and m.near(1e-3) == [], (L, pl, w)
                assert (w < G.WEAK_EDGE) == pl.flag_list           # (exact, so 0.99e-8 and 1.01e-8 are on their sides for certain)
            elif m.near(1e-3) or 0.9e-8 <= w <= 1.1e-8:
                left_out.append(r)
            else:
                (flagged if w < G.WEAK_EDGE else clear).append(r)
        assert tuple(flagged) == G.WEAK_FLAGGED and tuple(left_out) == G.WEAK_LEFT_OUT, (L, flagged, left_out)
        assert len(flagged) >= 5 and len(clear) >= 5 and len(left_out) <= 0.05 * rows.shape[0]
        assert expect.tolist() == [r for r, pl in zip(pos, batch) if pl.flag_list]
    rows, expect = G.planted(llr, batch, 1)
    assert expect.size == 0 and np.array_equal(rows, llr)                      # (list size 1: no such guard, the rows stay ordinary)


def m_leaf(m, leaf):
    return m.weak[leaf]
