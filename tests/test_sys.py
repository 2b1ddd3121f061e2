"""CPU suite of systematic coding: the library's host tables (polar_get_sys_info, polar_get_sys_positions: no GPU is
needed) against the plain numpy evaluation of the four definitions in tests/sys_numpy.py, and the properties of that evaluation."""
import numpy as np
import pytest

import polar_amd
import sys_numpy as M

CONSTRUCTED = [(n, crc) for n in range(5, 12) for crc in (0, 8, 16, 32) if (1 << n) // 2 + crc <= (1 << n)]
RANDOM_SEEDS = range(12)


_mirror = M.mirror_of


def _same(g, m):
    depth, swapped = g.systematic_info()
    pos, par = g.systematic_positions()
    assert (depth, swapped) == (m.depth, m.n_swapped)
    assert (pos == m.pos).all() and (par == m.par).all()
    return depth, swapped


random_code, swapped_code = M.random_code, M.swapped_code


def _properties(m, seed=1, rows=6):
    msg = np.random.default_rng(seed).integers(0, 2, (rows, m.K)).astype(np.uint8)
    coded, u = m.encode_systematic(msg)
    assert (coded[:, m.pos] == msg).all()
    assert not m.syndrome(m.place(u)).any()
    assert (m.message(u) == msg).all()
    any_u = np.random.default_rng(seed + 1).integers(0, 2, (rows, m.K)).astype(np.uint8)      # not only precoded words
    assert (m.message(any_u) == m.encode(any_u)[:, m.pos]).all()
    assert len(set(m.pos.tolist()) | set(m.par.tolist())) == m.Kp


@pytest.mark.parametrize("n,crc", CONSTRUCTED)
def test_constructed_codes(built_lib, n, crc):
    g = polar_amd.PolarCode(n, (1 << n) // 2, 0.32, crc)
    m = _mirror(g)
    depth, _ = _same(g, m)
    assert depth == 1
    _properties(m)


@pytest.mark.parametrize("n,K,crc", [(5, 1, 0), (6, 32, 32), (6, 1, 8), (5, 32, 0)])
def test_edge_sizes(built_lib, n, K, crc):
    g = polar_amd.PolarCode(n, K, 0.32, crc)
    m = _mirror(g)
    assert _same(g, m)[0] == 1
    _properties(m)


def test_mask_case_tables(built_lib, oracle_built):
    import mask_cases as MC
    tabs = MC.octet_codes(10)[:4] + MC.octet_codes(11)[:2] + list(MC.edge_masks().values()) + MC.soft_codes()[:4] + [MC.adaptive_case()]
    depths = []
    for t in tabs:
        g = t.handle()
        m = _mirror(g)
        depths.append(_same(g, m)[0])
        if t.n <= 10:
            _properties(m, rows=3)
    print("depths on the mask-case tables:", sorted(set(depths)))


def test_random_sets_need_rounds(built_lib):
    depths = []
    for seed in RANDOM_SEEDS:
        g = random_code(seed)
        m = _mirror(g)
        depths.append(_same(g, m)[0])
        _properties(m)
    print("depths on random sets of N = 128:", depths)
    assert max(depths) >= 3 and max(depths) <= 7


def test_swapped_parity_positions(built_lib):
    g = swapped_code()
    m = _mirror(g)
    _, swapped = _same(g, m)
    assert swapped > 0
    _properties(m)


def test_tables_follow_the_crc_matrix(built_lib):
    """polar_set_crc_matrix drops the tables: the next call builds them for the new matrix."""
    g = swapped_code()
    before = g.systematic_positions()[1].copy()
    g.crc_matrix = np.zeros((g.crc_size, g.K), np.uint8)
    m = _mirror(g)
    _, swapped = _same(g, m)
    assert swapped == 0 and not (g.systematic_positions()[1] == before).all()
    assert sorted(g.systematic_positions()[1].tolist()) == sorted(m.bitrev[m.order[m.K:m.Kp]].tolist())


def test_table_build_is_quick_at_the_largest_length(built_lib):
    g = polar_amd.PolarCode(15, 1 << 14, 0.32, 16)
    depth, swapped = g.systematic_info()
    pos, par = g.systematic_positions()
    assert depth == 1 and swapped == 0
    assert len(set(pos.tolist()) | set(par.tolist())) == g.K + 16
