"""Systematic coding on the device (polar_encode_sys_batch[_dev], polar_sys_message_batch[_dev], polar_sys_soft_batch[_dev],
polar_synth_sys_llr_dev, polar_mc_batch_sys) against the numpy evaluation of tests/sys_numpy.py and against the library's own plain
calls. Shapes where the packed layout changes: N = 32 (a partial word), 64 (one word), 128 (the first cross-lane stage), 2048, 4096
(all 64 lanes), 8192 (two words a lane), 32768; K = 1; K' = N; batches that leave waves partly filled; a frozen set that needs several
rounds of T^-1; a code whose parity positions leave order[K .. K'). Above n = 11 nothing is compared with the mirror: properties only."""
import numpy as np
import pytest

import sys_numpy as M

pytestmark = pytest.mark.gpu
SENT = 0xA5
# (n, K, crc)
SMALL = [(5, 16, 0), (5, 1, 0), (6, 32, 8), (6, 32, 32), (7, 64, 8), (7, 64, 0), (9, 256, 32), (11, 1024, 16)]
LARGE = [(12, 2048, 16), (13, 4096, 16), (15, 16384, 32)]
BATCHES = (0, 1, 3, 65, 1000)


def _gpu(key):
    import polar_amd
    return polar_amd.PolarCode(key[0], key[1], 0.32, key[2])


def _deep_code():
    """The first seeded random set of N = 128 with a CRC whose T^-1 takes at least 3 rounds."""
    for seed in range(1, 12, 2):
        g = M.random_code(seed)
        if g.systematic_info()[0] >= 3:
            return g
    raise AssertionError("no random set with depth >= 3")


def _special(name):
    return _deep_code() if name == "deep" else M.swapped_code()


def _bits(seed, B, K):
    return np.random.default_rng(seed).integers(0, 2, (B, K)).astype(np.uint8)


def _check_encode(g, msg, m=None):
    coded, u = g.encode_systematic(msg)
    pos, _ = g.systematic_positions()
    assert coded.shape == (len(msg), g.N) and u.shape == msg.shape
    assert (coded[:, pos] == msg).all()
    if len(msg):
        assert (coded == g.encode(u)).all()
    if m is not None:
        assert (u == m.precode(msg)).all()
    assert (g.systematic_message(u) == msg).all()                       # 3. round trip
    return coded, u


# ---- 1. exact encode, 3. round trip --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SMALL)
def test_encode_equals_the_mirror(built_lib, key):
    g = _gpu(key)
    m = M.mirror_of(g)
    for B in BATCHES if key[0] in (5, 7, 11) else (1, 65):
        _check_encode(g, _bits(10 + B, B, g.K), m)


@pytest.mark.parametrize("name", ["deep", "swapped"])
def test_encode_on_the_special_codes(built_lib, name):
    g = _special(name)
    depth, swapped = g.systematic_info()
    assert depth >= 3 if name == "deep" else swapped > 0
    m = M.mirror_of(g)
    for B in BATCHES:
        _check_encode(g, _bits(20 + B, B, g.K), m)


@pytest.mark.parametrize("key", LARGE)
def test_encode_properties_at_the_long_lengths(built_lib, key):
    g = _gpu(key)
    for B in (4,) if key[0] == 15 else (1, 3, 65):
        _check_encode(g, _bits(30 + B, B, g.K))


def test_encode_outputs_are_optional_and_bounded(built_lib):
    """Either output alone; sentinel-filled device outputs with a slack row stay untouched past B."""
    import torch
    g = _gpu((7, 64, 8))
    B = 67
    msg = _bits(3, B, g.K)
    coded, u = g.encode_systematic(msg)
    d_msg = torch.from_numpy(msg).cuda()
    for want_c, want_u in ((True, False), (False, True), (True, True)):
        d_c = torch.full((B + 1, g.N), SENT, dtype=torch.uint8, device="cuda")
        d_u = torch.full((B + 1, g.K), SENT, dtype=torch.uint8, device="cuda")
        g.encode_systematic_dev(d_msg.data_ptr(), B, d_c.data_ptr() if want_c else 0, d_u.data_ptr() if want_u else 0)
        torch.cuda.synchronize()
        c, uu = d_c.cpu().numpy(), d_u.cpu().numpy()
        assert (c[:B] == coded).all() if want_c else (c == SENT).all()
        assert (uu[:B] == u).all() if want_u else (uu == SENT).all()
        assert (c[B] == SENT).all() and (uu[B] == SENT).all()


# ---- 2. exact recovery for ANY u_info ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SMALL + LARGE)
def test_message_equals_encode_and_gather(built_lib, key):
    g = _gpu(key)
    pos, _ = g.systematic_positions()
    for B in (4,) if key[0] == 15 else ((1, 3, 65, 1000) if key[0] in (5, 7, 11) else (1, 65)):
        u = _bits(40 + B, B, g.K)
        assert (g.systematic_message(u) == g.encode(u)[:, pos]).all()
    assert g.systematic_message(np.zeros((0, g.K), np.uint8)).shape == (0, g.K)


@pytest.mark.parametrize("name", ["deep", "swapped"])
def test_message_on_the_special_codes(built_lib, name):
    g = _special(name)
    m = M.mirror_of(g)
    for B in (1, 3, 65, 1000):
        u = _bits(50 + B, B, g.K)
        got = g.systematic_message(u)
        assert (got == g.encode(u)[:, g.systematic_positions()[0]]).all() and (got == m.message(u)).all()


def test_message_in_place_slack_and_back_to_back(built_lib):
    """In place; sentinel-filled output with a slack row; two calls on one stream with nothing between them."""
    import torch
    g = _gpu((11, 1024, 16))
    pos, _ = g.systematic_positions()
    B = 131
    u = _bits(6, B, g.K)
    want = g.encode(u)[:, pos]
    d_u = torch.from_numpy(u).cuda()
    d_m = torch.full((B + 1, g.K), SENT, dtype=torch.uint8, device="cuda")
    d_m2 = torch.full((B + 1, g.K), SENT, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        g.systematic_message_dev(d_u.data_ptr(), B, d_m.data_ptr(), stream=st)
        g.systematic_message_dev(d_m.data_ptr(), B, d_m2.data_ptr(), stream=st)          # reads what the first call wrote
    st.synchronize()
    got, got2 = d_m.cpu().numpy(), d_m2.cpu().numpy()
    assert (got[:B] == want).all() and (got[B] == SENT).all()
    assert (got2[:B] == g.encode(want)[:, pos]).all() and (got2[B] == SENT).all()
    g.systematic_message_dev(d_u.data_ptr(), B, d_u.data_ptr())                          # in place
    torch.cuda.synchronize()
    assert (d_u.cpu().numpy() == want).all()


def _noisy(g, coded, ebno_db, seed):
    s = g.snr_sqrt_linear(ebno_db)
    z = np.random.default_rng(seed).standard_normal(coded.shape)
    return -4.0 * s * (s * (2.0 * coded - 1.0) + np.sqrt(0.5) * z)


def _clean(coded, seed):
    """Strong noiseless rows whose magnitudes are spread: a single magnitude would make a tie row."""
    mag = np.random.default_rng(seed).uniform(6.0, 14.0, coded.shape)
    return (1.0 - 2.0 * coded) * mag


def test_message_of_a_whole_list(built_lib):
    """The cand [B][L][K] of decode_scl_llr_list go through as B L rows."""
    g = _gpu((8, 128, 8))
    pos, _ = g.systematic_positions()
    coded, _ = g.encode_systematic(_bits(7, 24, g.K))
    cand = g.decode_scl_llr_list(_noisy(g, coded, 1.0, 8), 4)[0]
    got = g.systematic_message(cand)
    assert got.shape == cand.shape
    assert (got.reshape(-1, g.K) == g.encode(cand.reshape(-1, g.K))[:, pos]).all()


# ---- 4. every decoder with systematic=True -------------------------------------------------------------------------------------------
def _decoders(g):
    out = [("scl L=%d" % L, lambda llr, sysm, L=L: g.decode_scl_llr(llr, L, systematic=sysm)) for L in (1, 4, 32)]
    out.append(("scl f32", lambda llr, sysm: g.decode_scl_llr(llr.astype(np.float32), 4, systematic=sysm)))
    if g.crc_size:
        out.append(("adaptive", lambda llr, sysm: g.decode_scl_llr_adaptive(llr, (1, 4), systematic=sysm)[0]))
        out.append(("sc-flip", lambda llr, sysm: g.decode_sc_flip(llr, 4, systematic=sysm)[0]))
    out.append(("scan", lambda llr, sysm: g.decode_scan(llr, 2, systematic=sysm)[0]))
    return out


@pytest.mark.parametrize("which", [(8, 128, 8), (7, 64, 0), "swapped", "mask"])
def test_decoders_with_systematic(built_lib, oracle_built, which):
    if which == "mask":                                 # a decodable frozen set (no weak leaf) on which T^-1 takes several rounds
        import mask_cases as MC
        g = next(h for h in (t.handle() for t in MC.soft_codes()) if h.systematic_info()[0] > 1)
    else:
        g = M.swapped_code() if which == "swapped" else _gpu(which)
    msg = _bits(9, 48, g.K)
    coded, _ = g.encode_systematic(msg)
    noisy, clean = _noisy(g, coded, 1.0, 10), _clean(coded, 11)
    for name, dec in _decoders(g):
        plain = dec(noisy, False)
        assert (dec(noisy, True) == g.systematic_message(plain)).all(), name
        assert (dec(clean, True) == msg).all(), name
    print("%s: %d of 48 noisy rows decode to the sent message at L = 32" % (which, int((_decoders(g)[2][1](noisy, True) == msg).all(axis=1).sum())))


def test_scan_with_systematic_returns_message_llrs(built_lib):
    g = _gpu((8, 128, 8))
    pos, _ = g.systematic_positions()
    coded, _ = g.encode_systematic(_bits(12, 16, g.K))
    llr = _noisy(g, coded, 2.0, 13)
    out, info_llr, ext, ok, nit = g.decode_scan(llr, 3)
    out_s, msg_llr, ext_s, ok_s, nit_s = g.decode_scan(llr, 3, systematic=True)
    assert np.array_equal(ext, ext_s) and np.array_equal(ok, ok_s) and np.array_equal(nit, nit_s)
    assert (out_s == g.systematic_message(out)).all()
    assert np.array_equal((llr + ext)[:, pos].view(np.uint64), msg_llr.view(np.uint64))


# ---- 5. soft message outputs ---------------------------------------------------------------------------------------------------------
def _widen(a, fmt):
    if fmt == "bf16":
        return (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    if fmt == "f16":
        return a.view(np.float16).astype(np.float64)
    return a.astype(np.float64)


@pytest.mark.parametrize("fmt", ["f64", "f32", "f16", "bf16"])
@pytest.mark.parametrize("key", [(5, 16, 0), (9, 256, 32)])
def test_soft_outputs_are_the_gathered_sums(built_lib, key, fmt):
    import torch
    g = _gpu(key)
    pos, _ = g.systematic_positions()
    B = 37
    rng = np.random.default_rng(14)
    x = rng.standard_normal((B, g.N)) * 7
    llr = {"f64": x, "f32": x.astype(np.float32), "f16": x.astype(np.float16).view(np.uint16),
           "bf16": (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)}[fmt]
    ext = rng.standard_normal((B, g.N)) * 3
    ext[rng.random((B, g.N)) < 0.1] = np.inf
    want = (_widen(llr, fmt) + ext)[:, pos]
    assert np.isinf(want).any()
    got = g.systematic_soft(llr, ext, fmt)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    d_llr, d_ext = torch.from_numpy(llr.view(np.int16) if llr.dtype == np.uint16 else llr).cuda(), torch.from_numpy(ext).cuda()
    d_out = torch.full((B + 1, g.K), -7.5, dtype=torch.float64, device="cuda")
    g.systematic_soft_dev(d_llr.data_ptr(), fmt, d_ext.data_ptr(), B, d_out.data_ptr())
    torch.cuda.synchronize()
    o = d_out.cpu().numpy()
    assert np.array_equal(o[:B].view(np.uint64), want.view(np.uint64)) and (o[B] == -7.5).all()


# ---- 6. the sweep against the composition of its parts ---------------------------------------------------------------------------------
def _synth_sys(g, seed, t0, B, point, constellation=0):
    import torch
    llr = torch.empty((B, g.N), dtype=torch.float64, device="cuda")
    msg = torch.empty((B, g.K), dtype=torch.uint8, device="cuda")
    u = torch.empty((B, g.K), dtype=torch.uint8, device="cuda")
    g.synth_sys_llr_dev(seed, t0, B, g.snr_sqrt_linear(point) if constellation == 0 else point, llr.data_ptr(), msg.data_ptr(), u.data_ptr(),
                        constellation=constellation)
    torch.cuda.synchronize()
    return llr, msg, u


@pytest.mark.parametrize("constellation", [0, "ask4-gray"])
def test_the_systematic_workload_is_the_plain_one_with_another_codeword(built_lib, constellation):
    """Trial t sends as message the info bits the plain workload draws for trial t, over the same noise: where the two codewords
    agree in all the bits of a channel use, the LLRs are the plain workload's bit for bit."""
    import torch
    g = _gpu((7, 64, 8))
    B, seed, t0, point = 130, 5, 95, 2.0
    llr, msg, u = _synth_sys(g, seed, t0, B, point, constellation)
    p_llr = torch.empty((B, g.N), dtype=torch.float64, device="cuda")
    p_info = torch.empty((B, g.K), dtype=torch.uint8, device="cuda")
    if constellation == 0:
        g.synth_llr_dev(seed, t0, B, g.snr_sqrt_linear(point), p_llr.data_ptr(), p_info.data_ptr())
    else:
        g.synth_bicm_llr_dev(constellation, seed, t0, B, point, p_llr.data_ptr(), p_info.data_ptr())
    torch.cuda.synchronize()
    msg, u, llr, p_llr = msg.cpu().numpy(), u.cpu().numpy(), llr.cpu().numpy(), p_llr.cpu().numpy()
    assert (msg == p_info.cpu().numpy()).all()
    coded, u_want = g.encode_systematic(msg)
    assert (u == u_want).all()
    nb = 1 if constellation == 0 else 2
    same = (coded == g.encode(msg)).reshape(B, g.N // nb, nb).all(axis=2).repeat(nb, axis=1)
    assert same.any() and not same.all()
    assert np.array_equal(llr[same].view(np.uint64), p_llr[same].view(np.uint64))
    assert (llr[~same] != p_llr[~same]).any()


def test_sweep_counters_equal_the_composition(built_lib):
    import torch
    import polar_amd
    g = _gpu((7, 64, 8))
    Ls, axis, T, stride, t0, seed = (1, 4), (1.0, 2.5), 300, 3, 40, 11
    stats = np.full((len(Ls), len(axis), polar_amd.SY_N), 7, np.uint64)
    g.mc_batch_sys(seed, t0, 0, stride, axis, Ls, np.ones((2, 2), np.uint8), stats)
    assert (stats == 7).all()                                           # T = 0 leaves stats alone
    enabled = np.array([[1, 1], [0, 1]], np.uint8)
    g.mc_batch_sys(seed, t0, T, stride, axis, Ls, enabled, stats)
    for li, L in enumerate(Ls):
        for ie, e in enumerate(axis):
            if not enabled[li, ie]:
                assert (stats[li, ie] == 7).all()
                continue
            llr, msg, u = _synth_sys(g, seed, t0, stride * T, e)
            llr, msg, u = llr[::stride].contiguous(), msg[::stride].contiguous(), u[::stride].contiguous()
            out = torch.empty((T, g.K), dtype=torch.uint8, device="cuda")
            mhat = torch.empty((T, g.K), dtype=torch.uint8, device="cuda")
            g.decode_scl_llr_dev(llr.data_ptr(), T, L, out.data_ptr())
            g.systematic_message_dev(out.data_ptr(), T, mhat.data_ptr())
            torch.cuda.synchronize()
            du, dm = (out != u).cpu().numpy(), (mhat != msg).cpu().numpy()
            assert (du.any(axis=1) == dm.any(axis=1)).all()            # a block error in the message exactly when there is one in u
            want = [T, int(du.any(axis=1).sum()), int(dm.sum()), int(du.sum())]
            print("L = %d, %.1f dB:" % (L, e), want)
            assert (stats[li, ie] - 7).tolist() == want


def test_sweep_counters_do_not_depend_on_the_chunks(built_lib):
    """The same trials in one chunk and in chunks of 7 (45 trials: six whole chunks and one of 3; three enabled cells: the trial
    offset of a chunk restarts twice), and split into the even and the odd ones: counts of the same trials, equal as integers."""
    import polar_amd
    g = _gpu((7, 64, 8))
    Ls, axis, stride, t0, seed = (1, 4), (1.0, 2.5), 3, 40, 11
    enabled = np.array([[1, 1], [0, 1]], np.uint8)

    def run(T, t0, stride):
        stats = np.full((len(Ls), len(axis), polar_amd.SY_N), 7, np.uint64)
        g.mc_batch_sys(seed, t0, T, stride, axis, Ls, enabled, stats)
        assert (stats[1, 0] == 7).all()                                # the disabled cell is untouched
        return stats
    whole = run(45, t0, stride)
    g.debug_set("list_chunk_cw", 7)
    try:
        chunked = run(45, t0, stride)
    finally:
        g.debug_set("list_chunk_cw", 0)
    print("one chunk", whole.tolist(), "chunks of 7", chunked.tolist())
    assert (whole[enabled == 1, polar_amd.SY_RUN] == 7 + 45).all()
    assert whole.tolist() == chunked.tolist()
    # even and odd trials
    halves = (run(22, t0, 2 * stride) - 7) + (run(22, t0 + stride, 2 * stride) - 7)
    assert halves.tolist() == (run(44, t0, stride) - 7).tolist()


# ---- 7. the point of it all ------------------------------------------------------------------------------------------------------------
def test_message_ber_is_below_u_domain_ber(built_lib):
    """N = 128, K = 64, no CRC, L = 1, 2.5 dB, 4000 trials: a numpy min-sum SC model gives BIT_MSG / BIT_U = 0.43 on such trials."""
    import polar_amd
    g = _gpu((7, 64, 0))
    r = g.systematic_stats([2.5], [1], max_runs=4000, max_err=10 ** 9, batch=4000)
    s = r["stats"][0, 0]
    print("BLER %.4f, message BER %.5f, u-domain BER %.5f, ratio %.3f" % (r["bler"][0, 0], r["ber_msg"][0, 0], r["ber_u"][0, 0],
                                                                        s[polar_amd.SY_BIT_MSG] / max(1, s[polar_amd.SY_BIT_U])))
    assert s[polar_amd.SY_RUN] == 4000 and s[polar_amd.SY_ERR] > 0
    assert s[polar_amd.SY_BIT_MSG] < s[polar_amd.SY_BIT_U]


# ---- the C++ mirror --------------------------------------------------------------------------------------------------------------------
CPP_MAIN = r"""
#include <cstdio>
#include "PolarCode.hpp"
static void row(const std::vector<uint8_t> &v) { for (uint8_t b : v) putchar('0' + b); putchar('\n'); }
int main(int argc, char **argv) {
    // argv[1]: B messages of 32 bytes, argv[2]: B rows of 64 doubles; prints coded, u_info, the messages of u_info, the decoded messages, pos
    PolarCode code(6, 32, 0.32, 8);
    std::vector<uint8_t> msg;
    std::vector<double> llr;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    for (int c; (c = fgetc(f)) != EOF;) msg.push_back((uint8_t)c);
    fclose(f);
    f = fopen(argv[2], "rb");
    if (!f) return 2;
    double x;
    while (fread(&x, sizeof x, 1, f) == 1) llr.push_back(x);
    fclose(f);
    std::vector<uint8_t> u;
    row(code.encode_systematic(msg, &u));
    row(u);
    row(code.systematic_message(u));
    row(code.decode_scl_llr_systematic(llr, 4));
    for (uint16_t p : code.systematic_positions()) printf("%d ", (int)p);
    putchar('\n');
    return 0;
}
"""


def test_cpp_mirror(built_lib, tmp_path):
    import ctypes as C
    import os
    import subprocess
    from polar_amd import build
    C.CDLL(None).srand(C.c_uint(1))                    # (the CRC matrix of polar_create is drawn from rand(): a fresh process starts at seed 1)
    g = _gpu((6, 32, 8))
    B = 9
    msg = _bits(15, B, g.K)
    coded, u = g.encode_systematic(msg)
    llr = _noisy(g, coded, 2.0, 16)
    msg.tofile(str(tmp_path / "msg.bin"))
    llr.tofile(str(tmp_path / "llr.bin"))
    (tmp_path / "main.cpp").write_text(CPP_MAIN)
    exe = str(tmp_path / "sys_main")
    here = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", build.INC, "-I", os.path.join(here, "cpp"), str(tmp_path / "main.cpp"),
                           "-o", exe, "-L", here, "-lpolar_amd", "-Wl,-rpath," + here,
                           "-Wl,-rpath," + (build._torch_lib() or "/opt/rocm/lib"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path / "msg.bin"), str(tmp_path / "llr.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()

    def bits(a):
        return "".join(str(int(v)) for v in a.reshape(-1))
    assert lines[0] == bits(coded) and lines[1] == bits(u) and lines[2] == bits(msg)
    assert lines[3] == bits(g.decode_scl_llr(llr, 4, systematic=True))
    assert [int(v) for v in lines[4].split()] == g.systematic_positions()[0].tolist()


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(built_lib):
    import ctypes as C
    import polar_amd
    g = _gpu((7, 64, 8))
    L = polar_amd.lib()
    buf = np.zeros(4 * g.N, np.uint8)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert L.polar_encode_sys_batch(g._h, ptr, C.c_long(1), None, None) == -1
    assert L.polar_encode_sys_batch(g._h, None, C.c_long(1), ptr, None) == -1
    assert L.polar_encode_sys_batch(g._h, ptr, C.c_long(-1), ptr, None) == -1
    assert L.polar_sys_message_batch(g._h, ptr, C.c_long(-1), ptr) == -1
    assert L.polar_sys_message_batch(None, ptr, C.c_long(1), ptr) == -1
    assert L.polar_sys_soft_batch_dev(g._h, ptr, C.c_int(9), ptr, C.c_long(1), ptr, None) == -1
    assert L.polar_synth_sys_llr_dev(g._h, C.c_int(polar_amd.RX_MLC | polar_amd.ASK4_GRAY), C.c_uint64(1), C.c_uint64(0), C.c_long(1),
                                     C.c_double(1.0), ptr, None, None, None) == -1
    assert L.polar_synth_sys_llr_dev(g._h, C.c_int(99), C.c_uint64(1), C.c_uint64(0), C.c_long(1), C.c_double(1.0), ptr, None, None, None) == -1
    with pytest.raises(polar_amd.PolarError):
        g.mc_batch_sys(1, 0, 10, 0, [1.0], [1], [1], np.zeros((1, 1, polar_amd.SY_N), np.uint64))      # stride < 1
    with pytest.raises(polar_amd.PolarError):
        g.mc_batch_sys(1, 0, 10, 1, [1.0], [65], [1], np.zeros((1, 1, polar_amd.SY_N), np.uint64))     # list size out of range
    assert L.polar_encode_sys_batch(g._h, ptr, C.c_long(0), ptr, None) == 0                            # B = 0: nothing to do
