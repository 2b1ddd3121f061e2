"""16-bit channel LLRs (POLAR_LLR_F16 / POLAR_LLR_BF16 of include/polar_amd.h): the numpy widening the tests feed the oracle
with, and the test rows both suites share. Widening is exact: every binary16 / bfloat16 value is a double."""
import numpy as np

F16_MAX = 65504.0                      # 0x7BFF
BF16_MAX_PATTERN = 0x7F7F              # (2 - 2^-7) 2^127
BF16_INF_PATTERN = 0x7F80


def widen_f16(a):
    """binary16 values (np.float16, or their uint16 patterns) -> the same values as float64."""
    a = np.asarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.float16)
    assert a.dtype == np.float16
    return a.astype(np.float64)


def widen_bf16(u16):
    """bfloat16 bit patterns (uint16) -> the same values as float64: a bfloat16 is the upper half of a float32."""
    u16 = np.asarray(u16)
    assert u16.dtype == np.uint16
    return (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def to_bf16_patterns(x):
    """float64 / float32 values -> bfloat16 patterns by truncation of the float32."""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def planted_rows(llr):
    """The oracle's synth_llr rows [B >= 2][N >= 16] as (float16 array, bfloat16 patterns), with the special values planted:
    row 0 holds +0, -0, a binary16 subnormal (6e-8), the bfloat16 subnormal 0x0001 (bf16 rows; 9.2e-41 is below binary16's
    range), the largest finite value of the format and +inf; row 1 is the row scaled by 2^-10 (many binary16 subnormals)."""
    llr = np.array(llr, np.float64)
    llr[1] *= 2.0 ** -10
    f16 = llr.astype(np.float16)
    bf = to_bf16_patterns(llr)
    f16[0, :5] = [0.0, -0.0, np.float16(6e-8), np.float16(F16_MAX), np.inf]
    bf[0, :7] = [0x0000, 0x8000, int(to_bf16_patterns(np.float32(6e-8))[0]), 0x0001, BF16_MAX_PATTERN, BF16_INF_PATTERN, 0x8001]
    assert f16[0, 2] != 0 and f16[0, 2] < 6.2e-5 and np.isfinite(f16[0, 3])
    return f16, bf
