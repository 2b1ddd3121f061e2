"""Symbol-domain BICM receiver, the parts that need no GPU: polar_modulate and the Constellation mirror against the numpy
restatement of PolarM/Constellation.m (tests/polarm_numpy.py), the argument refusals that are made before any device work,
and the declarations in include/polar_amd.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import polarm_numpy as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ask4-gray": 1, "ask8-gray": 2, "ask16-gray": 3, "bpsk": 4, "ask4-sp": 5, "ask8-sp": 6, "ask16-sp": 7}
# Constellation.m:23, 27, 31-32: the set-partition tables are the levels in ascending order (polarm_numpy.LEVELS holds the
# Gray tables and BPSK only; the tests add these three, written from the MATLAB text, for the duration of a test)
SP_LEVELS = {5: (list(range(-3, 4, 2)), 5.0), 6: (list(range(-7, 8, 2)), 21.0), 7: (list(range(-15, 16, 2)), 85.0)}
NEW_ENTRY_POINTS = ("polar_modulate", "polar_demap_bicm", "polar_demap_bicm_f32", "polar_demap_bicm_dev", "polar_demap_bicm_dev_f32",
                    "polar_decode_bicm_batch", "polar_decode_bicm_batch_f32", "polar_decode_bicm_batch_dev",
                    "polar_decode_bicm_batch_dev_f32", "polar_synth_bicm_sym_dev")


@pytest.fixture
def numpy_levels(monkeypatch):
    for cid, v in SP_LEVELS.items():
        monkeypatch.setitem(PM.LEVELS, cid, v)
    return PM


def test_new_entry_points_are_declared_and_exported(built_lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polar_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(polar_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(built_lib)
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("name", sorted(NAMES))
def test_constellation_attributes_match_numpy(built_lib, numpy_levels, name):
    import polar_amd
    c = polar_amd.Constellation(name)
    pts, nb = numpy_levels.constellation(NAMES[name])
    assert c.name == name and c.id == NAMES[name] and c.n_bits == nb and c.n_sym == len(pts) == 1 << nb
    assert c.points.shape == (c.n_sym,) and c.points.dtype == np.float64
    # numpy sums the squares pairwise, the library in symbol order (Constellation.m:80 does not say): 1 ulp
    assert (np.abs(c.points - pts) <= np.spacing(np.abs(pts))).all()
    assert abs(np.mean(c.points ** 2) - 1.0) < 1e-15


@pytest.mark.parametrize("name", sorted(NAMES))
def test_modulate_matches_numpy_without_a_device(built_lib, numpy_levels, name):
    import polar_amd
    c = polar_amd.Constellation(name)
    rng = np.random.default_rng(NAMES[name])
    for N in (1024, 1000, 7, 4):
        bits = rng.integers(0, 2, (5, N)).astype(np.uint8)
        got = c.modulate(bits)
        assert got.shape == (5, N // c.n_bits)
        for b in range(5):
            want, sym = numpy_levels.modulate(bits[b], NAMES[name])
            assert (got[b] == c.points[sym]).all()                          # the symbol indices, exactly
            assert (np.abs(got[b] - want) <= np.spacing(np.abs(want))).all()  # the values: the points' 1 ulp
        assert (c.modulate(bits[0]) == got[0]).all()                        # one row


def test_refusals_that_need_no_device(built_lib):
    import polar_amd
    L = polar_amd.lib()
    dp, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    bits = np.zeros(16, np.uint8)
    sym = np.zeros(16)
    E_ARG = -1
    mod = lambda cid, b, N, B, s: L.polar_modulate(C.c_int(cid), b, C.c_int(N), C.c_long(B), s)
    pb, ps = bits.ctypes.data_as(u8p), sym.ctypes.data_as(dp)
    assert mod(3, pb, 16, 1, ps) == 0
    assert mod(3, pb, 16, 0, ps) == 0                                       # B = 0: nothing to do
    for bad in ((0, pb, 16, 1, ps), (8, pb, 16, 1, ps), (0x103, pb, 16, 1, ps), (3, None, 16, 1, ps), (3, pb, 16, 1, None),
                (3, pb, 0, 1, ps), (3, pb, 16, -1, ps)):
        assert mod(*bad) == E_ARG, bad
        assert L.polar_last_error()
    with pytest.raises(polar_amd.PolarError):
        polar_amd.Constellation("qam16")
    with pytest.raises(polar_amd.PolarError):
        polar_amd.Constellation(0)
    c = polar_amd.Constellation("ask16-gray")
    y = np.zeros((2, 4))
    # refused before any device work: n0, both outputs NULL, unknown ids, negative B, NULL y
    for n0 in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(polar_amd.PolarError, match="n0"):
            c.compute_llr_bicm(y, n0)
    dem = lambda cid, yp, N, B, n0, l, p: L.polar_demap_bicm(C.c_int(cid), yp, C.c_int(N), C.c_long(B), C.c_double(n0), l, p)
    py = y.ctypes.data_as(dp)
    out = np.zeros((2, 16))
    po = out.ctypes.data_as(dp)
    for bad in ((3, py, 16, 2, 0.1, None, None), (0, py, 16, 2, 0.1, po, None), (9, py, 16, 2, 0.1, po, None),
                (3, None, 16, 2, 0.1, po, None), (3, py, 16, -2, 0.1, po, None), (3, py, 0, 2, 0.1, po, None)):
        assert dem(*bad) == E_ARG, bad
    assert dem(3, py, 16, 0, 0.1, po, None) == 0                            # B = 0 needs no device either
    with pytest.raises(polar_amd.PolarError):
        c.compute_llr_bicm(y, 0.1, block_length=24)                         # 24 // 4 != 4 symbols per row
    # decode from symbols: row width, constellation, n0, list size — all before the device is touched
    g = polar_amd.PolarCode(5, 16, 0.32, 0)
    good = np.zeros((3, 8))
    for bad_y in (np.zeros((3, 32)), np.zeros((3, 7)), np.zeros(9), np.zeros((2, 3, 8))):
        with pytest.raises(polar_amd.PolarError, match="decode_bicm"):
            g.decode_bicm(bad_y, 0.1, "ask16-gray", 1)
    for kw in (dict(n0=0.0), dict(n0=float("nan")), dict(n0=-0.5), dict(c=0), dict(c=8), dict(L=0), dict(L=65), dict(L=-1)):
        with pytest.raises(polar_amd.PolarError):
            g.decode_bicm(good, kw.get("n0", 0.1), kw.get("c", "ask16-gray"), kw.get("L", 1))
    assert g.decode_bicm(np.zeros((0, 8)), 0.1, "ask16-gray", 4).shape == (0, 16)          # B = 0
    assert g.decode_bicm(np.zeros((0, 8), np.float32), 0.1, "ask16-gray", 4).shape == (0, 16)
    assert (g.frozen_bits.sum() == 16)                                      # the handle is still usable
