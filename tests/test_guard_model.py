"""CPU suite: the conditions on the inputs that tests/test_gpu_fallback_rows.py rests on, proven on the oracle and numpy alone, so
that the model of tests/guard_numpy.py — and not what a kernel happens to flag — decides which rows are expected in the fallback
set. If a row breaks a condition here, choose another seed or block in guard_numpy's table; the GPU assertions are not widened.

Not proven here (DESIGN.md "Which rows take the fallback pass"): that no ordinary row of a list decode comes within the |x| < 40
window at a node BELOW its first descent — those nodes depend on the paths' decisions. That rests on the window's width alone
(about 1e7 node evaluations in the whole GPU file times a few 1e-10 of probability mass each)."""
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
        b = G.B_LARGE if n == 11 else G.B
        llr, _ = o.synth_llr(G.CODES[key], 0, b, o.snr_sqrt_linear(G.EBNO))
        llr.setflags(write=False)
        _cache[key] = (o, Code(o), llr)
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
