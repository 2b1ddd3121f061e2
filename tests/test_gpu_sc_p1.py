"""GPU suite: decode_sc_p1 against the oracle, the same doubles, through both of its kernels (sc_p1_kernel: one lane per codeword,
state in an HBM scratch; sc_p1_lat_kernel: one codeword per wave, state in LDS) at the shapes they special-case: n = 1 and n = 2,
K = 1 and K = N, the LDS gate between N = 4096 and N = 8192, a wave that decodes a second and a third codeword (registers and
LDS carry over), the lane kernel's grid-stride loop and ragged last waves. tests/test_p1_oracle.py pins the oracle to the numpy
restatement of the MATLAB formulas on the rows used here. Rows are those of p1_rows.rows without p0."""
import numpy as np
import pytest

import p1_rows
from golden_util import both_kernels

pytestmark = pytest.mark.gpu


def _check(o, g, p1, what, want=None):
    """Both kernels forced in turn (golden_util.both_kernels asserts they agree), then the oracle row by row: NaN positions
    apart from the values."""
    got = both_kernels(g, lambda: g.decode_sc_p1(p1))
    assert got.shape == (p1.shape[0], o.K)
    if want is None:
        want = np.stack([o.decode_sc_p1(p1[i]) for i in range(p1.shape[0])])
    bad = p1_rows.rows_that_differ(got, want)
    assert bad.size == 0, f"{bad.size}/{p1.shape[0]} rows differ from the oracle (first {bad[:8]}) {what}"


@pytest.mark.parametrize("n,K", [(1, 1), (1, 2), (2, 1), (2, 2), (2, 4), (3, 1), (3, 4), (3, 8), (4, 1), (4, 8), (4, 16)])
def test_tiny_block_lengths(built_lib, oracle_built, n, K):
    """n = 1 (the leaf is the only layer), n = 2 (no generic partial-sum walk), nothing frozen (K = N), one unfrozen leaf (K = 1).
    70 rows: a ragged second wave in the lane kernel, 70 waves in the other."""
    o, g = p1_rows.pair(n, K, 0)
    p1, _ = p1_rows.rows(o, 70, 1.0)
    _check(o, g, p1, (n, K))


@pytest.mark.parametrize("n,K", [(11, 1024), (12, 2048), (13, 4096)])
def test_lds_gate(built_lib, oracle_built, n, K):
    """The one-codeword-per-wave kernel's state is 4 N doubles + N bytes of LDS: two waves per CU at N = 2048, one at N = 4096;
    N = 8192 does not fit, and forcing the kernel there must fall through to the lane kernel and still be right. The "lat_waves"
    hook says which of the two the forced call took."""
    o, g = p1_rows.pair(n, K, 0)
    p1, _ = p1_rows.rows(o, 5, 1.0)
    _check(o, g, p1, (n, K))
    g.debug_set("lat_max_b", 1 << 40)
    g.decode_sc_p1(p1)
    waves = g.debug_get("lat_waves")
    g.debug_set("lat_max_b", 0)
    assert (waves == 5) if n <= 12 else (waves == 0), (n, waves)


def test_a_waves_second_and_third_codeword(built_lib, oracle_built):
    """N = 4096: one wave per CU, so 2 CUs + 3 codewords give every wave a second codeword and three waves a third one. The left
    leaf's decision lives in a register and the partial sums in LDS across codewords; every seventh row is a degenerate one."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    o, g = p1_rows.pair(12, 2048, 0)
    p1, _ = p1_rows.rows(o, 2 * cus + 3, 1.0, every=7)
    _check(o, g, p1, p1.shape[0])


def test_lane_kernel_grid_stride_and_ragged_waves(built_lib, oracle_built):
    """More codewords than 16 waves per CU hold lanes: the second trip of sc_p1_kernel's loop, with a ragged last wave. The rows
    are drawn from a pool of 4096 distinct ones (degenerate rows every 97), so only the pool goes through the oracle. The
    loop's stride is 64 * 16 * CUs codewords, a multiple of 4096 whenever CUs is a multiple of 4: plain tiling would hand every
    lane on its second trip the row it decoded on its first, and state or input left over from the first trip would go unseen.
    So the pool index moves on by one per stride: each lane's second row is its first row's neighbour in the pool."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    o, g = p1_rows.pair(2, 3, 0)
    pool, _ = p1_rows.rows(o, 4096, 1.0, every=97)
    want_pool = np.stack([o.decode_sc_p1(pool[i]) for i in range(4096)])
    B = 64 * 16 * cus + 69
    stride = 64 * 16 * cus
    idx = (np.arange(B) + np.arange(B) // stride) % 4096
    assert (idx[stride:] != idx[:B - stride]).all()
    _check(o, g, pool[idx], B, want_pool[idx])
    for b in (1, 63, 64, 65, 129):
        _check(o, g, pool[:b], b, want_pool[:b])
