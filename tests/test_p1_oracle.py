"""CPU suite: the specification of the probability-domain decoders, pinned before the device is compared with it.
test_gpu_scl_p1.py and test_gpu_sc_p1.py compare the kernels of polar_kernels_p1.hip bit for bit with oracle_lib.Oracle on
degenerate rows (ties, zeros, underflow); here the oracle itself is shown to be the reference on those rows:
  decode_scl_p1 == the unmodified reference build (oracle/_ref), where it was built;
  decode_sc_p1  == tests/polarm_numpy.py, an evaluation of the MATLAB formulas that shares no code with the C restatement.
Exact equality everywhere: only + - * / and comparisons are involved."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import p1_rows
import polarm_numpy as M

libc = C.CDLL(None)
LIST_SIZES = [1, 2, 3, 4, 5, 7, 8, 12, 16, 20, 32, 33, 64]


@pytest.mark.skipif(not oracle_lib.have_reference(), reason="oracle/_ref not built here")
@pytest.mark.parametrize("n,K,crc", [(1, 1, 0), (2, 3, 0), (3, 5, 1), (4, 11, 2), (5, 16, 4), (6, 30, 4), (7, 64, 8), (9, 256, 8),
                                     (12, 2048, 16)])
def test_oracle_decode_scl_p1_equals_the_reference_on_every_row_family(oracle_built, n, K, crc):
    """Ordinary rows at 1 dB and all six degenerate rows, every list size (odd ones, lists larger than 2^K): no row left out."""
    libc.srand(1)
    r = oracle_lib.Reference(n, K, 0.32, crc)
    o = p1_rows.oracle(n, K, crc)
    assert (r.frozen() == o.frozen()).all() and (r.order() == o.order()).all() and (r.crc_matrix() == o.crc_matrix()).all()
    p1, p0 = p1_rows.rows(o, 8 if n >= 12 else 40, 1.0)
    for L in LIST_SIZES:
        for i in range(p1.shape[0]):
            assert (o.decode_scl_p1(p1[i], p0[i], L) == r.decode_scl_p1(p1[i], p0[i], L)).all(), (L, i)


def _numpy_sc_p1(o, p1):
    with np.errstate(all="ignore"):
        u, _ = M.polar_decode(p1, o.frozen().astype(np.float64))
    return u[o.order()[: o.K]]


@pytest.mark.parametrize("n,K", [(1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (2, 4), (3, 1), (3, 4), (3, 8), (4, 1), (4, 8), (4, 16),
                                 (11, 1024), (12, 2048), (13, 4096)])
def test_oracle_decode_sc_p1_equals_numpy_on_the_edge_rows(oracle_built, n, K):
    """The six degenerate rows and their ordinary neighbours, at every code the device tests use."""
    o = p1_rows.oracle(n, K, 0)
    p1, _ = p1_rows.rows(o, 10, 1.0)
    got = np.stack([o.decode_sc_p1(p1[i]) for i in range(p1.shape[0])])
    want = np.stack([_numpy_sc_p1(o, p1[i]) for i in range(p1.shape[0])])
    bad = p1_rows.rows_that_differ(got, want)
    assert bad.size == 0, bad
    assert (got[0] == 0.5).all()                 # the all-0.5 row: sign(0) = 0 at every unfrozen leaf (PolarCode.m:873)
