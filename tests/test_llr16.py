"""16-bit channel LLRs, the part that needs no GPU: the ABI exports the format entry points, an unknown format code is refused
before any device is touched, and the numpy widening the GPU tests feed the oracle with is exact for all 65 536 patterns of
each format (checked against a decode of the bit fields that shares nothing with numpy's conversions)."""
import ctypes as C

import numpy as np
import pytest

from llr16_util import planted_rows, to_bf16_patterns, widen_bf16, widen_f16


def test_new_symbols_are_exported(built_lib):
    import polar_amd
    L = polar_amd.lib()
    for name in ("polar_decode_scl_llr_batch_fmt", "polar_decode_scl_llr_batch_dev_fmt",
                 "polar_decode_scl_llr_batch", "polar_decode_scl_llr_batch_f32",
                 "polar_decode_scl_llr_batch_dev", "polar_decode_scl_llr_batch_dev_f32"):
        assert hasattr(L, name), name
    assert (polar_amd.LLR_F64, polar_amd.LLR_F32, polar_amd.LLR_F16, polar_amd.LLR_BF16) == (0, 1, 2, 3)
    assert hasattr(polar_amd.PolarCode, "decode_scl_llr_dev_fmt")
    from polar_amd import build
    hdr = open(build.INC + "/polar_amd.h").read()
    for line in ("#define POLAR_LLR_F64  0", "#define POLAR_LLR_F32  1", "#define POLAR_LLR_F16  2", "#define POLAR_LLR_BF16 3"):
        assert line in hdr, line


@pytest.mark.parametrize("fmt", [-1, 4])
def test_unknown_format_is_an_argument_error_without_a_device(built_lib, fmt):
    """POLAR_E_ARG with a message, for the host-pointer and the device-pointer form: the check precedes everything that needs
    a device (this test runs where there is none)."""
    import polar_amd
    g = polar_amd.PolarCode(6, 20, 0.32, 3)
    L = polar_amd.lib()
    rows = np.zeros((2, 64), np.float64)
    out = np.zeros((2, 20), np.uint8)
    rc = L.polar_decode_scl_llr_batch_fmt(g._h, C.c_void_p(rows.ctypes.data), C.c_int(fmt), C.c_long(2), C.c_int(1),
                                          C.c_void_p(out.ctypes.data))
    assert rc == -1
    msg = L.polar_last_error().decode()
    assert "format" in msg and str(fmt) in msg, msg
    rc = L.polar_decode_scl_llr_batch_dev_fmt(g._h, C.c_void_p(rows.ctypes.data), C.c_int(fmt), C.c_long(2), C.c_int(1),
                                              C.c_void_p(out.ctypes.data), C.c_void_p(0), C.c_void_p(0))
    assert rc == -1
    assert "format" in L.polar_last_error().decode()
    # the Python layer refuses an unknown name, and float rows offered as bfloat16 patterns (those come as uint16)
    for bad, arr in (("fp8", rows), ("bf16", rows), ("bf16", rows.astype(np.float16))):
        try:
            g.decode_scl_llr(arr, 1, fmt=bad)
            refused = False
        except polar_amd.PolarError:
            refused = True
        assert refused, bad
    g.close()


def _decode_fields(u, eb, mb):
    """All patterns `u` of a 16-bit format with eb exponent and mb mantissa bits -> float64, from the bit fields with exact
    integer / power-of-two arithmetic (ldexp of an integer significand)."""
    u = u.astype(np.int64)
    s = (u >> 15) & 1
    e = (u >> mb) & ((1 << eb) - 1)
    m = u & ((1 << mb) - 1)
    bias = (1 << (eb - 1)) - 1
    sig = np.where(e == 0, m, m + (1 << mb)).astype(np.float64)
    val = np.ldexp(sig, (np.maximum(e, 1) - bias - mb).astype(np.int32))
    top = e == (1 << eb) - 1
    val = np.where(top & (m == 0), np.inf, val)
    val = np.where(top & (m != 0), np.nan, val)
    return np.where(s == 1, -val, val)


@pytest.mark.parametrize("name,eb,mb", [("f16", 5, 10), ("bf16", 8, 7)])
def test_numpy_widening_is_exact_for_every_pattern(name, eb, mb):
    u = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    got = widen_f16(u) if name == "f16" else widen_bf16(u)
    want = _decode_fields(u, eb, mb)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all() and nan.sum() == 2 * ((1 << mb) - 1)
    # same doubles, bit for bit (signed zeros included)
    assert (got[~nan].view(np.uint64) == want[~nan].view(np.uint64)).all()
    # and back: narrowing the double gives the pattern again
    back = got.astype(np.float16).view(np.uint16) if name == "f16" else to_bf16_patterns(got)
    assert (back[~nan] == u[~nan]).all()
    # the subnormals are there and non-zero: 2^mb - 1 of each sign
    sub = (((u >> mb) & ((1 << eb) - 1)) == 0) & ((u & ((1 << mb) - 1)) != 0)
    assert sub.sum() == 2 * ((1 << mb) - 1) and (got[sub] != 0).all()
    assert abs(got[1]) == (2.0 ** -24 if name == "f16" else 2.0 ** -133)


def test_planted_rows_hold_the_special_values():
    rng = np.random.default_rng(5)
    f16, bf = planted_rows(rng.normal(2.0, 2.0, (3, 64)))
    w16, wbf = widen_f16(f16), widen_bf16(bf)
    assert w16[0, 0] == 0 and not np.signbit(w16[0, 0]) and w16[0, 1] == 0 and np.signbit(w16[0, 1])
    assert 0 < w16[0, 2] < 2.0 ** -14 and w16[0, 3] == 65504.0 and w16[0, 4] == np.inf
    assert wbf[0, 0] == 0 and np.signbit(wbf[0, 1]) and wbf[0, 3] == 2.0 ** -133 and wbf[0, 6] == -(2.0 ** -133)
    assert wbf[0, 4] == (2.0 - 2.0 ** -7) * 2.0 ** 127 and wbf[0, 5] == np.inf
    assert np.isfinite(w16[1:]).all() and np.isfinite(wbf[1:]).all()
    # row 1: many binary16 subnormals
    assert ((np.abs(w16[1]) < 2.0 ** -14) & (w16[1] != 0)).sum() >= 1
