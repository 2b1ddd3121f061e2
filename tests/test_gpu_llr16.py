"""GPU suite: fp16 / bf16 channel LLRs at the boundary of decode_scl_llr (POLAR_LLR_F16 / POLAR_LLR_BF16). The contract is the
float form's: out == decode_scl_llr(widen(llr)) bit for bit, widen = the exact value of each 16-bit pattern as a double. Every
check is == on decoded bits (and path metrics) against the oracle, or against the float64 call, fed the widened rows."""
import os
import subprocess

import numpy as np
import pytest

from llr16_util import planted_rows, widen_bf16, widen_f16
from test_gpu_parity import _pair, both_kernels, both_l1_kernels

pytestmark = pytest.mark.gpu

FORMATS = ("f16", "bf16")


def _rows(o, seed, B):
    """{"f16": (host array, widened), "bf16": ...} from the oracle's synthetic rows with the special values planted."""
    llr, _ = o.synth_llr(seed, 0, B, o.snr_sqrt_linear(1.5))
    f16, bf = planted_rows(llr)
    return {"f16": (f16, widen_f16(f16)), "bf16": (bf, widen_bf16(bf))}


def _host(g, fmt, a, L):
    return g.decode_scl_llr(a, L) if fmt == "f16" else g.decode_scl_llr(a, L, fmt="bf16")


def _dev_tensor(a, extra=0):
    """The 16-bit patterns of `a` in device memory (a flat int16 tensor, `extra` elements longer, rows starting at element
    `extra`): what a torch.float16 / torch.bfloat16 tensor holds."""
    import torch
    flat = np.ascontiguousarray(a).view(np.int16).reshape(-1)
    t = torch.zeros(flat.size + extra, dtype=torch.int16, device="cuda")
    t[extra:] = torch.from_numpy(flat.copy()).cuda()
    return t


def _dev(g, fmt, t, B, L, K, pm=False, offset=0):
    import torch
    out = torch.zeros((B, K), dtype=torch.uint8, device="cuda")
    d_pm = torch.zeros(B, dtype=torch.float64, device="cuda") if pm else None
    g.decode_scl_llr_dev_fmt(t.data_ptr() + 2 * offset, fmt, B, L, out.data_ptr(), pm_ptr=d_pm.data_ptr() if pm else 0)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (d_pm.cpu().numpy() if pm else None)


@pytest.mark.parametrize("n,K,crc,L", [(6, 20, 3, 1), (9, 256, 8, 8), (11, 1024, 16, 1), (11, 1024, 16, 32)])
def test_parity_per_format(built_lib, oracle_built, n, K, crc, L):
    """Both formats, host pointer and device pointer, latency and batch kernels; with d_pm requested the path metrics are those
    of the float64 call on the widened rows."""
    import torch
    o, g = _pair(n, K, crc)
    B = 40
    rows = _rows(o, 515, B)
    for fmt in FORMATS:
        a, wide = rows[fmt]
        want = o.decode_scl_llr(wide, L)
        got = both_kernels(g, lambda: _host(g, fmt, a, L)) if L <= 8 else _host(g, fmt, a, L)
        assert (got == want).all(), (fmt, "host", np.nonzero((got != want).any(axis=1))[0])
        t = _dev_tensor(a)
        if L <= 8:
            got = both_kernels(g, lambda: _dev(g, fmt, t, B, L, K)[0])
        else:
            got = _dev(g, fmt, t, B, L, K)[0]
        assert (got == want).all(), (fmt, "device", np.nonzero((got != want).any(axis=1))[0])
        # path metrics: the general kernel (list size 1 included), against the float64 entry point on the widened rows
        got, pm = _dev(g, fmt, t, B, L, K, pm=True)
        d64 = torch.tensor(wide, device="cuda")
        out64 = torch.zeros((B, K), dtype=torch.uint8, device="cuda")
        pm64 = torch.zeros(B, dtype=torch.float64, device="cuda")
        g.decode_scl_llr_dev(d64.data_ptr(), B, L, out64.data_ptr(), pm_ptr=pm64.data_ptr())
        torch.cuda.synchronize()
        assert (got == want).all() and (out64.cpu().numpy() == want).all(), fmt
        assert (pm.view(np.uint64) == pm64.cpu().numpy().view(np.uint64)).all(), fmt
    # the same from torch's own 16-bit tensors (the patterns reinterpreted, as a receiver holds them)
    out = torch.zeros((B, K), dtype=torch.uint8, device="cuda")
    for fmt, dt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        a, wide = rows[fmt]
        tt = _dev_tensor(a).view(dt).reshape(B, 1 << n)
        assert tt.dtype == dt and tt.element_size() == 2
        g.decode_scl_llr_dev_fmt(tt.data_ptr(), fmt, B, L, out.data_ptr())
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == o.decode_scl_llr(wide, L)).all(), fmt


@pytest.mark.parametrize("fmt", FORMATS)
def test_unfused_conversion_pass(built_lib, oracle_built, fmt):
    """List of 32 with the "no_fuse_front" knob: the rows go through ed_front_kernel's 16-bit instantiation (the conversion pass
    of its own, otherwise taken only by codes without a staged prefix) instead of the prefix kernel's first pass."""
    o, g = _pair(11, 1024, 16)
    B = 40
    a, wide = _rows(o, 515, B)[fmt]
    want = o.decode_scl_llr(wide, 32)
    t = _dev_tensor(a)
    g.debug_set("no_fuse_front", 1)
    try:
        got_h = _host(g, fmt, a, 32)
        got_d = _dev(g, fmt, t, B, 32, 1024)[0]
    finally:
        g.debug_set("no_fuse_front", 0)
    assert (got_h == want).all() and (got_d == want).all(), fmt
    assert (_dev(g, fmt, t, B, 32, 1024)[0] == want).all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_list_size_one_schedules(built_lib, oracle_built, fmt):
    """List size 1 on a ragged batch: the folded schedule (eight 16-bit values = one 16-byte load of the caller's rows), the
    sc_no_fold schedule (front pass), and rows that start one element off a 16-byte boundary (the converted copy)."""
    o, g = _pair(11, 1024, 0)
    B = 203
    a, wide = _rows(o, 77, B)[fmt]
    want = o.decode_scl_llr(wide, 1)
    t = _dev_tensor(a)
    got = both_l1_kernels(g, lambda: _dev(g, fmt, t, B, 1, 1024)[0])
    assert (got == want).all(), ("fold", np.nonzero((got != want).any(axis=1))[0])
    assert (both_l1_kernels(g, lambda: _host(g, fmt, a, 1)) == want).all()
    g.debug_set("sc_no_fold", 1)
    try:
        got = both_l1_kernels(g, lambda: _dev(g, fmt, t, B, 1, 1024)[0])
    finally:
        g.debug_set("sc_no_fold", 0)
    assert (got == want).all(), ("no fold", np.nonzero((got != want).any(axis=1))[0])
    t1 = _dev_tensor(a, extra=1)                     # one element longer than the batch: the offset rows stay inside it
    assert (t1.data_ptr() + 2) % 16 != 0
    got = both_l1_kernels(g, lambda: _dev(g, fmt, t1, B, 1, 1024, offset=1)[0])
    assert (got == want).all(), ("offset", np.nonzero((got != want).any(axis=1))[0])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("L", [1, 4, 32])
def test_flagged_rows_take_the_fallback_pass(built_lib, oracle_built, fmt, L):
    """Every row holds an exact zero: every codeword is flagged and decoded by the LLR-domain kernel from the 16-bit rows."""
    o, g = _pair(9, 256, 8)
    B = 70
    a, _ = _rows(o, 31, B)[fmt]
    a = a.copy()
    a[np.arange(B), (7 * np.arange(B)) % 512] = 0
    wide = widen_f16(a) if fmt == "f16" else widen_bf16(a)
    assert ((wide == 0).sum(axis=1) >= 1).all()
    want = o.decode_scl_llr(wide, L)
    got = both_kernels(g, lambda: _host(g, fmt, a, L)) if L <= 8 else _host(g, fmt, a, L)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0]
    t = _dev_tensor(a)
    assert (_dev(g, fmt, t, B, L, 256)[0] == want).all()


@pytest.mark.parametrize("L", [1, 4])
def test_pipelined_host_path(built_lib, oracle_built, L):
    """fp16 rows through the chunked host pipeline (2 bytes per element in the slot and chunk arithmetic), B no multiple of the
    chunk: the bits of the single-launch path, in more than one chunk."""
    o, g = _pair(8, 128, 4)
    B = 333
    a, wide = _rows(o, 11, B)["f16"]
    want = o.decode_scl_llr(wide, L)
    g.debug_set("host_pipe_min_bytes", -1)
    single = g.decode_scl_llr(a, L)
    assert g.debug_get("host_chunks") == 0
    g.debug_set("host_pipe_min_bytes", 1)
    g.debug_set("host_ramp", -1)
    g.debug_set("host_lanes", 2)
    g.debug_set("host_chunk_bytes", 64 * 256 * 2)            # 64 rows of 2-byte elements
    try:
        got = g.decode_scl_llr(a, L)
        chunks = g.debug_get("host_chunks")
    finally:
        for k in ("host_pipe_min_bytes", "host_ramp", "host_lanes", "host_chunk_bytes"):
            g.debug_set(k, 0)
    assert chunks == -(-B // 64) and chunks > 1, chunks
    assert (got == single).all() and (single == want).all()


def test_no_allocation_after_reserve(built_lib, oracle_built):
    """polar_reserve's promise covers the two new formats: device-resident calls within (B, L) leave the allocation counter alone
    (rows 16-byte aligned or not, with and without the path-metric output)."""
    import torch
    o, g = _pair(9, 256, 8)
    B = 1200
    g.reserve(B, 32)
    t = torch.zeros(B * 512 + 1, dtype=torch.int16, device="cuda")
    t[:] = 0x4000                                        # 2.0 in both formats
    out = torch.zeros((B, 256), dtype=torch.uint8, device="cuda")
    pm = torch.zeros(B, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    a0 = g.debug_get("allocs")
    for fmt in FORMATS:
        for L in (32, 1, 2, 4, 8, 16):
            for b in (B, 1):
                g.decode_scl_llr_dev_fmt(t.data_ptr(), fmt, b, L, out.data_ptr())
                g.decode_scl_llr_dev_fmt(t.data_ptr(), fmt, b, L, out.data_ptr(), pm_ptr=pm.data_ptr())
        g.decode_scl_llr_dev_fmt(t.data_ptr() + 2, fmt, B, 1, out.data_ptr())
    torch.cuda.synchronize()
    assert g.debug_get("allocs") == a0


CPP_MAIN = r"""
#include <cstdio>
#include <vector>
#include "PolarCode.hpp"
int main(int argc, char **argv) {
    // argv[1] / argv[2]: files of binary16 / bfloat16 patterns, B rows of 1024; prints B lines of 512 bits for each
    PolarCode code(10, 512, 0.32, 0);
    const int fmts[2] = {POLAR_LLR_F16, POLAR_LLR_BF16};
    for (int k = 0; k < 2; ++k) {
        std::vector<uint16_t> v;
        FILE *f = fopen(argv[1 + k], "rb");
        if (!f) return 2;
        uint16_t x;
        while (fread(&x, sizeof x, 1, f) == 1) v.push_back(x);
        fclose(f);
        std::vector<uint8_t> out = code.decode_scl_llr_batch(v, fmts[k], 4);
        for (size_t i = 0; i < out.size(); ++i) { putchar('0' + out[i]); if (i % 512 == 511) putchar('\n'); }
    }
    std::vector<uint16_t> v(1024, 0x4000);
    try { code.decode_scl_llr_batch(v, POLAR_LLR_F32, 4); return 3; } catch (const std::out_of_range &) {} catch (const std::exception &) {}
    return 0;
}
"""


def test_cpp_mirror(built_lib, oracle_built, tmp_path):
    """A program written against polar_amd/cpp/PolarCode.hpp decodes 16-bit rows in both formats: the Python layer's bits."""
    from polar_amd import build
    o, g = _pair(10, 512, 0)
    B = 12
    rows = _rows(o, 5, B)
    for fmt in FORMATS:
        np.ascontiguousarray(rows[fmt][0]).view(np.uint16).tofile(str(tmp_path / (fmt + ".bin")))
    (tmp_path / "main.cpp").write_text(CPP_MAIN)
    exe = str(tmp_path / "llr16_main")
    here = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", build.INC, "-I", os.path.join(here, "cpp"), str(tmp_path / "main.cpp"),
                           "-o", exe, "-L", here, "-lpolar_amd", "-Wl,-rpath," + here,
                           "-Wl,-rpath," + (build._torch_lib() or "/opt/rocm/lib"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path / "f16.bin"), str(tmp_path / "bf16.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.array([[int(ch) for ch in line] for line in r.stdout.strip().splitlines()], np.uint8)
    assert got.shape == (2 * B, 512)
    for k, fmt in enumerate(FORMATS):
        want = _host(g, fmt, rows[fmt][0], 4)
        assert (want == o.decode_scl_llr(rows[fmt][1], 4)).all()
        assert (got[k * B:(k + 1) * B] == want).all(), fmt
