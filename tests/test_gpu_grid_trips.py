"""GPU suite: the later trips of the grid-stride loops of polar_kernels_rm.hip and polar_kernels_sys.hip. Every
kernel of both files walks the batch under a capped grid; tests/test_gpu_rm.py and tests/test_gpu_sys.py stop at 1000 rows, far below
the caps, so no lane of theirs goes round its row loop twice: the four rows in flight of rm_recover_kernel's SINGLE variant, the
`b += step` of its list-walking variant, the registers sys_precode_kernel keeps across trips. Here every batch exceeds the pass size
of its kernel, computed in the test from the launch formula and asserted, so a change of the launch geometry fails the test and
does not silently un-test the path.

The big comparisons stay on the device: inputs are drawn with torch, the expectation of recover is a restatement of §8k's definition
in three torch lines (not the kernel's organisation), and outputs are compared as 64-bit patterns there — one boolean and the first
offending row come back. Every case fills its output and a sentinel row on either side, asserts the sentinels, and calls twice back
to back on one stream."""
import warnings

import numpy as np
import pytest

import rm_cases as RC
import rm_numpy as M
import sys_numpy as SN

pytestmark = pytest.mark.gpu
SENT = -12345.678
SENT8 = 0xA5
ROWS_GRID = 8192                 # polar_kernels.h polar_rows_grid: blocks of the one-codeword-per-block kernels
SYS_WAVES = 16384                # polar_kernels_sys.hip kGridCap
SOFT_LANES = 8192 * 256          # polar_launch_sys_soft
SWEEP_BYTES = 512 << 20          # polar_host.h sweep_chunk's budget
_handles = {}


# ---- the launch formulas, restated ---------------------------------------------------------------------------------------------------
def pass_rows(N):
    """Rows one pass of rm_recover_kernel's grid covers (recover_launch): tpr lanes a row, 256 / tpr rows a block, gx blocks across a
    row, at most max(1, 16384 / gx) blocks of rows."""
    tpr = min(256, max(1, N // 2))
    rows_pb = 256 // tpr
    gx = -(-(N // 2) // tpr)
    return max(1, 16384 // gx) * rows_pb


def sys_pass_rows(N):
    """Codewords one pass of sys_precode_kernel / sys_message_kernel covers (sys_grid): 16 384 waves of G codewords."""
    W = max(1, N // 64)
    return SYS_WAVES * (1 if W >= 64 else 64 // W)


def test_the_formulas_give_the_documented_pass_sizes():
    assert [pass_rows(N) for N in (2, 4, 16, 32, 1024, 2048, 32768)] == [2097152 * 2, 16384 * 128, 16384 * 32, 262144, 8192, 4096, 256]
    assert [sys_pass_rows(N) for N in (32, 64, 2048, 4096, 32768)] == [64 * 16384, 64 * 16384, 2 * 16384, 16384, 16384]


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------
def _rm_design(n, K, crc, E, scheme, ebno):
    """from_gauss_approx_rm at phi_dx = 1e-4, once per shape (only recover and the workload run on these handles here)."""
    key = (n, K, crc, E, scheme, ebno)
    if key not in _handles:
        import polar_amd
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", polar_amd.PolarWeakLeavesWarning)
            _handles[key] = polar_amd.PolarCode.from_gauss_approx_rm(1 << n, K, E, scheme, ebno, crc, phi_dx=RC.PHI_DX)
    return _handles[key]


def _plain(n, K, crc, sel=None, known=None):
    import polar_amd
    g = polar_amd.PolarCode(n, K, 0.32, crc)
    if sel is not None:
        g.set_rate_match(sel, known)
    return g


def _values(B, E, seed, dtype):
    """Received rows drawn on the device: every magnitude from 1e-3 to 1e3, a seventh -0.0, +inf and -inf among them (in float16
    large values overflow to infinities and small ones become subnormals as well)."""
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    v = torch.randn((B, E), generator=gen, device="cuda", dtype=torch.float64)
    v *= 10.0 ** torch.randint(-3, 3, (B, E), generator=gen, device="cuda").to(torch.float64)
    u = torch.rand((B, E), generator=gen, device="cuda")
    v[u < 1 / 7] = -0.0
    v[(u >= 0.3) & (u < 0.3 + 1 / 11)] = float("inf")
    v[(u >= 0.5) & (u < 0.5 + 1 / 13)] = float("-inf")
    v[0, 0] = -0.0
    v = v.to(dtype)
    assert bool(((v == 0) & torch.signbit(v)).any()) and bool(torch.isposinf(v).any()) and bool(torch.isneginf(v).any())
    return v


def _want(rx, sel, known, N):
    """§8k's definition of recover on the device: +0.0, plus the widened sources in ascending e, 1000.0 at a known position."""
    import torch
    B, E = rx.shape
    wide = rx.to(torch.float64)
    sel = np.asarray(sel, np.int64)
    if len(np.unique(sel)) == E:
        want = torch.zeros((B, N), dtype=torch.float64, device="cuda")
        want[:, torch.from_numpy(sel).cuda()] = 0.0 + wide
    else:
        assert N <= E < 2 * N and (sel == np.arange(E) % N).all()
        want = 0.0 + wide[:, :N]
        want[:, :E - N] += wide[:, N:]
    if known is not None and np.asarray(known).any():
        want[:, torch.from_numpy(np.flatnonzero(known)).cuda()] = 1000.0
    return want


def _first_bad_row(got, want):
    """-1 if the rows are equal as 64-bit patterns (a NaN — inf - inf of a doubled position — equals any NaN), else the first row
    that is not."""
    import torch
    bad = (got.view(torch.int64) != want.view(torch.int64)) & ~(torch.isnan(got) & torch.isnan(want))
    rows = bad.any(dim=1)
    return int(rows.nonzero()[0]) if bool(rows.any()) else -1


def _recover_and_compare(g, rx, fmt, want, offs=(0,)):
    """rate_recover_dev twice into a sentinel-filled buffer, at a 16-byte-aligned start and (off = 1) at one that is only 8-byte
    aligned; `want` a torch tensor or a numpy array [B, N]."""
    import torch
    B, N = want.shape
    buf = torch.empty(((B + 2) * N + 1,), dtype=torch.float64, device="cuda")
    for off in offs:
        buf.fill_(SENT)
        out = buf[off + N: off + N + B * N]
        assert (out.data_ptr() % 16 == 0) == (off == 0)
        g.rate_recover_dev(rx.data_ptr(), fmt, B, out.data_ptr())
        g.rate_recover_dev(rx.data_ptr(), fmt, B, out.data_ptr())
        torch.cuda.synchronize()
        if isinstance(want, np.ndarray):
            got = out.reshape(B, N).cpu().numpy()
            ok = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
            assert ok.all(), "row %d differs" % int(np.flatnonzero(~ok.all(axis=1))[0])
        else:
            bad = _first_bad_row(out.reshape(B, N), want)
            assert bad == -1, "row %d differs (off %d)" % (bad, off)
        assert bool((buf[:off + N] == SENT).all()) and bool((buf[off + N + B * N:] == SENT).all())


def _zeros_are_positive(want):
    import torch
    return not bool(((want == 0) & torch.signbit(want)).any())


# ---- 1. SINGLE, one row a block: four rows in flight, then a ragged second iteration ------------------------------------------------
@pytest.mark.parametrize("fmt", ["f16", "f64"])
@pytest.mark.parametrize("scheme", ["shorten", "puncture"])
def test_single_variant_second_iteration(built_lib, scheme, fmt):
    """n = 11, E = 1536, B = 5 P + 3 = 20 483: iteration one has all four rows valid in every block, iteration two has r = 0 valid
    everywhere and r = 1 in three blocks only. Shorten in f16 once more into an output that is only 8-byte aligned (VEC = false)."""
    import torch
    n, N, E = 11, 2048, 1536
    P = pass_rows(N)
    B = 5 * P + 3
    assert P == 4096 and B > 4 * P and B == 20483
    g = _rm_design(n, 768, 16, E, scheme, 1.5)
    sel, known, short = g.rate_match_info()
    assert short == 1000.0 and len(np.unique(sel)) == E and bool(known.any()) == (scheme == "shorten")
    rx = _values(B, E, 1, torch.float16 if fmt == "f16" else torch.float64)
    want = _want(rx, sel, known, N)
    assert _zeros_are_positive(want)
    _recover_and_compare(g, rx, fmt, want, offs=(0, 1) if (scheme, fmt) == ("shorten", "f16") else (0,))


# ---- 2. SINGLE, sixteen rows a block --------------------------------------------------------------------------------------------------
def test_single_variant_with_several_rows_a_block(built_lib):
    import torch
    n, N, E = 5, 32, 24
    P = pass_rows(N)
    B = 5 * P + 19
    assert P == 262144 and B > 4 * P
    sel, known = M.pattern(n, E, "puncture")
    g = _plain(n, 8, 8, sel)
    rx = _values(B, E, 2, torch.float64)
    want = _want(rx, sel, known, N)
    assert _zeros_are_positive(want)
    _recover_and_compare(g, rx, "f64", want)


# ---- 3. the list-walking variant --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,E,extra", [(11, 3072, 3), (5, 33, 19)])
def test_list_walking_variant_second_trip(built_lib, n, E, extra):
    import torch
    N = 1 << n
    P = pass_rows(N)
    B = P + extra
    assert B > P
    sel, known = M.pattern(n, E, "repeat")
    g = _plain(n, N // 2, 0, sel)
    rx = _values(B, E, 3, torch.float64)
    want = _want(rx, sel, known, N)
    assert bool(torch.isnan(want).any())                       # (inf - inf at a doubled position: any NaN for a NaN)
    _recover_and_compare(g, rx, "f64", want)


# ---- 4. NR's scattered sel ---------------------------------------------------------------------------------------------------------------
def test_single_variant_with_a_scattered_pattern(built_lib):
    import polar_amd
    import torch
    n, N, E, Kp = 11, 2048, 1536, 784
    P = pass_rows(N)
    B = 4 * P + 3
    assert B > 4 * P
    g = _rm_design(n, 768, 16, E, "nr", 1.5)
    sel, known = polar_amd.rate_match_pattern(n, E, "nr", Kp)
    sel_h, known_h, _ = g.rate_match_info()
    assert (sel == sel_h).all() and (known == known_h).all() and known.sum() == N - E
    assert (sel == M.pattern(n, E, "nr", Kp)[0]).all() and (np.diff(sel.astype(np.int64)) != 1).any()
    rx = _values(B, E, 4, torch.float16)
    _recover_and_compare(g, rx, "f16", _want(rx, sel, known, N))


# ---- 5. the ends of the shape range, small batches -------------------------------------------------------------------------------------
def _rx_np(seed, B, E):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((B, E)) * 10.0 ** rng.integers(-3, 3, (B, E))
    flat = v.reshape(-1)
    flat[rng.integers(0, flat.size, max(1, flat.size // 7))] = -0.0
    flat[rng.integers(0, flat.size, max(1, flat.size // 11))] = np.inf
    flat[rng.integers(0, flat.size, max(1, flat.size // 13))] = -np.inf
    flat[0] = -0.0
    return v


def _tiny_cases():
    import polar_amd
    rng = np.random.default_rng(5)
    out = [("n1 one sent, one punctured", _plain(1, 1, 0), np.array([1], np.uint16), None)]
    # n = 2: position 3 known (leaf 3 alone lies above it and is frozen on this handle), position 1 punctured
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", polar_amd.PolarWeakLeavesWarning)
        g2 = polar_amd.PolarCode.from_tables(2, 2, 0, np.array([1, 0, 0, 1], np.uint8), np.array([1, 2, 0, 3], np.uint16))
    out.append(("n2 known", g2, np.array([2, 0], np.uint16), np.array([0, 0, 0, 1], np.uint8)))
    out.append(("n4 single", _plain(4, 8, 0), rng.permutation(16)[:12].astype(np.uint16), None))
    out.append(("n4 lists", _plain(4, 8, 0), rng.integers(0, 14, 20).astype(np.uint16), None))
    return out


def test_the_smallest_codes(built_lib):
    """n = 1, 2, 4 (tpr = 1, 2, 8) with hand-written patterns, B = 1, 3, 65, against rm_numpy.recover."""
    import torch
    for name, g, sel, known in _tiny_cases():
        g.set_rate_match(sel, known)
        assert min(256, max(1, g.N // 2)) == {2: 1, 4: 2, 16: 8}[g.N]
        kn = np.zeros(g.N, np.uint8) if known is None else known
        for B in (1, 3, 65):
            rx = _rx_np(B, B, len(sel))
            with np.errstate(invalid="ignore"):
                want = M.recover(rx, sel, kn)
            assert (want[:, M.punctured(g.n, sel, kn)].view(np.uint64) == 0).all(), name
            _recover_and_compare(g, torch.from_numpy(rx).cuda(), "f64", want, offs=(0, 1))


def test_the_largest_pattern(built_lib):
    """n = 15 with E = 8 N = 262 144 (sel[e] = e mod N), the largest E the check admits: eight sources per position."""
    import torch
    n, N = 15, 32768
    sel = (np.arange(8 * N) % N).astype(np.uint16)
    g = _plain(n, 16384, 0, sel)
    with pytest.raises(Exception):
        g.set_rate_match(np.concatenate([sel, sel[:1]]))
    for B in (1, 3, 65):
        rx = _rx_np(B, B, 8 * N)
        with np.errstate(invalid="ignore"):
            want = M.recover(rx, sel, np.zeros(N, np.uint8))
        _recover_and_compare(g, torch.from_numpy(rx).cuda(), "f64", want)


# ---- 6. select ---------------------------------------------------------------------------------------------------------------------------
def test_rate_match_second_trip(built_lib):
    import torch
    n, N, E, B = 5, 32, 24, ROWS_GRID + 70
    assert B > ROWS_GRID
    sel, _ = M.pattern(n, E, "puncture")
    g = _plain(n, 8, 8, sel)
    coded = torch.randint(0, 2, (B, N), dtype=torch.uint8, device="cuda")
    buf = torch.full((B + 2, E), SENT8, dtype=torch.uint8, device="cuda")
    g.rate_match_dev(coded.data_ptr(), B, buf[1:].data_ptr())
    g.rate_match_dev(coded.data_ptr(), B, buf[1:].data_ptr())
    torch.cuda.synchronize()
    assert bool((buf[1:B + 1] == coded[:, torch.from_numpy(sel.astype(np.int64)).cuda()]).all())
    assert bool((buf[0] == SENT8).all()) and bool((buf[B + 1] == SENT8).all())


# ---- 7. the workloads ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(5, 8, 8, 24, "puncture", 2.0), (5, 8, 8, 33, "repeat", 2.0)], ids=["E24", "E33-odd"])
def test_synth_rm_second_trip(built_lib, oracle_built, key):
    """synth_rm_llr_dev (draw, encode, select, channel: each under polar_rows_grid) at B = 8192 + 70 from trial 95, against the
    oracle's info bits and encoder and the C shim's noise on every row; E = 33 ends on the z0 of a last pair."""
    import torch
    c = RC.case(key)
    g = c.handle()
    B, t0, E, K = ROWS_GRID + 70, 95, c.E, c.K
    assert B > ROWS_GRID
    rx, info = c.workload(np.arange(t0, t0 + B), ebno=2.0)
    s = g.snr_sqrt_linear_rm(2.0)
    assert s == M.snr_sqrt_linear_rm(K, E, 2.0)
    d_rx = torch.full((B + 2, E), 7.0, dtype=torch.float64, device="cuda")
    d_info = torch.full((B + 2, K), SENT8, dtype=torch.uint8, device="cuda")
    g.synth_rm_llr_dev(RC.SEED, t0, B, s, d_rx[1:].data_ptr(), d_info[1:].data_ptr())
    g.synth_rm_llr_dev(RC.SEED, t0, B, s, d_rx[1:].data_ptr(), d_info[1:].data_ptr())
    torch.cuda.synchronize()
    h_rx, h_info = d_rx.cpu().numpy(), d_info.cpu().numpy()
    bad = np.flatnonzero((h_rx[1:B + 1].view(np.uint64) != rx.view(np.uint64)).any(axis=1) | (h_info[1:B + 1] != info).any(axis=1))
    assert bad.size == 0, bad[:8]
    assert (h_rx[[0, B + 1]] == 7.0).all() and (h_info[[0, B + 1]] == SENT8).all()


def test_synth_sys_second_trip(built_lib):
    """synth_sys_llr_dev (sys_draw_kernel, the precode, sys_channel_kernel) at B = 8192 + 70, held to what tests/test_gpu_sys.py holds
    it to at B = 130: the messages are the plain workload's info bits, u_info is the precode of them, and wherever the systematic and
    the plain codeword agree the LLRs are the plain workload's bit for bit."""
    import torch
    g = _plain(5, 16, 0)
    B, seed, t0, point = ROWS_GRID + 70, 5, 95, 2.0
    assert B > ROWS_GRID
    s = g.snr_sqrt_linear(point)
    llr = torch.full((B + 1, g.N), 7.0, dtype=torch.float64, device="cuda")
    msg = torch.full((B + 1, g.K), SENT8, dtype=torch.uint8, device="cuda")
    u = torch.full((B + 1, g.K), SENT8, dtype=torch.uint8, device="cuda")
    p_llr = torch.empty((B, g.N), dtype=torch.float64, device="cuda")
    p_info = torch.empty((B, g.K), dtype=torch.uint8, device="cuda")
    for _ in range(2):
        g.synth_sys_llr_dev(seed, t0, B, s, llr.data_ptr(), msg.data_ptr(), u.data_ptr())
    g.synth_llr_dev(seed, t0, B, s, p_llr.data_ptr(), p_info.data_ptr())
    torch.cuda.synchronize()
    assert bool((llr[B] == 7.0).all()) and bool((msg[B] == SENT8).all()) and bool((u[B] == SENT8).all())
    msg, u, llr, p_llr = msg[:B].cpu().numpy(), u[:B].cpu().numpy(), llr[:B].cpu().numpy(), p_llr.cpu().numpy()
    assert (msg == p_info.cpu().numpy()).all()
    m = SN.mirror_of(g)
    assert (u == m.precode(msg)).all()
    coded = m.encode(u)
    assert (coded[:, g.systematic_positions()[0]] == msg).all()
    same = coded == g.encode(msg)
    assert same[ROWS_GRID:].any() and not same[ROWS_GRID:].all()
    assert np.array_equal(llr[same].view(np.uint64), p_llr[same].view(np.uint64))
    # (where the codewords differ the sign of the noiseless part differs: the LLR is the plain one's with the other coded bit)
    assert (llr[~same] != p_llr[~same]).any()


# ---- 8. the sweeps ---------------------------------------------------------------------------------------------------------------------------
def _one_chunk(T, per):
    """sweep_chunk puts all T trials into one chunk (a fresh handle has no "list_chunk_cw" set): min(T, 512 MiB / per) == T."""
    return SWEEP_BYTES // per >= T


def test_mc_batch_rm_second_trip(built_lib):
    """T = 8192 + 70 trials at stride 3 in one chunk (N = 32, E = 24: 520 bytes a trial against the sweep's 512 MiB): the counters
    equal the sum of two calls over the same trials split 4131 / 4131, each of which runs single-trip kernels that
    tests/test_gpu_rm.py holds to the oracle."""
    import polar_amd
    c = RC.case((5, 8, 8, 24, "puncture", 2.0))
    g = c.handle()
    T, stride, t0 = ROWS_GRID + 70, 3, 37
    half = T // 2
    assert T > ROWS_GRID and 2 * half == T and half < ROWS_GRID
    assert _one_chunk(T, c.N * 8 + c.N + c.E * 9 + 2 * c.K)

    def run(t0, T):
        stats = np.zeros((1, 1, polar_amd.RM_N), np.uint64)
        g.mc_batch_rm(RC.SEED, t0, T, stride, [c.ebno], [1], [1], stats)
        return stats[0, 0]
    whole, a, b = run(t0, T), run(t0, half), run(t0 + half * stride, half)
    print("whole", whole.tolist(), "halves", a.tolist(), b.tolist())
    assert whole[polar_amd.RM_RUN] == T and 0 < whole[polar_amd.RM_ERR] < T
    assert whole.tolist() == (a + b).tolist()


def test_mc_batch_sys_second_trip(built_lib):
    import polar_amd
    g = _plain(5, 16, 0)
    T, stride, t0, seed = ROWS_GRID + 70, 3, 40, 11
    half = T // 2
    assert T > ROWS_GRID and 2 * half == T
    assert _one_chunk(T, g.N * 8 + g.N + 5 * g.K)

    def run(t0, T):
        stats = np.zeros((1, 1, polar_amd.SY_N), np.uint64)
        g.mc_batch_sys(seed, t0, T, stride, [2.0], [1], [1], stats)
        return stats[0, 0]
    whole, a, b = run(t0, T), run(t0, half), run(t0 + half * stride, half)
    print("whole", whole.tolist(), "halves", a.tolist(), b.tolist())
    assert whole[polar_amd.SY_RUN] == T and 0 < whole[polar_amd.SY_ERR] < T
    assert whole.tolist() == (a + b).tolist()


# ---- 9. the packed systematic kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,crc,extra", [(12, 2048, 16, 5), (5, 16, 0, 70)], ids=["n12-G1", "n5-G64"])
def test_precode_and_message_second_trip(built_lib, n, K, crc, extra):
    """encode_systematic_dev / systematic_message_dev with more codewords than one pass of 16 384 waves holds (one codeword a wave at
    N = 4096, 64 at N = 32): the mirror on rows 0 .. 63 and on every second-trip row; on the device, for EVERY row, the message at
    the systematic positions of the codeword and back out of systematic_message(u_info)."""
    import torch
    g = _plain(n, K, crc)
    P = sys_pass_rows(g.N)
    B = P + extra
    assert B > P and P == SYS_WAVES * max(1, min(64, 4096 // g.N))
    pos = torch.from_numpy(g.systematic_positions()[0].astype(np.int64)).cuda()
    msg = torch.randint(0, 2, (B, K), dtype=torch.uint8, device="cuda")
    coded = torch.full((B + 2, g.N), SENT8, dtype=torch.uint8, device="cuda")
    u = torch.full((B + 2, K), SENT8, dtype=torch.uint8, device="cuda")
    back = torch.full((B + 2, K), SENT8, dtype=torch.uint8, device="cuda")
    for _ in range(2):
        g.encode_systematic_dev(msg.data_ptr(), B, coded[1:].data_ptr(), u[1:].data_ptr())
        g.systematic_message_dev(u[1:].data_ptr(), B, back[1:].data_ptr())
    torch.cuda.synchronize()
    for buf in (coded, u, back):
        assert bool((buf[0] == SENT8).all()) and bool((buf[B + 1] == SENT8).all())
    bad = (coded[1:B + 1][:, pos] != msg).any(dim=1) | (back[1:B + 1] != msg).any(dim=1)
    assert not bool(bad.any()), "row %d" % int(bad.nonzero()[0])
    m = SN.mirror_of(g)
    rows = np.concatenate([np.arange(64), np.arange(P, B)])
    idx = torch.from_numpy(rows).cuda()
    h_msg = msg[idx].cpu().numpy()
    want_c, want_u = m.encode_systematic(h_msg)
    assert (u[1:][idx].cpu().numpy() == want_u).all() and (coded[1:][idx].cpu().numpy() == want_c).all()
    assert (m.message(want_u) == h_msg).all()


def test_soft_outputs_second_trip(built_lib):
    """systematic_soft_dev at B K just above 8192 blocks of 256 lanes, against llr[pos] + ext[pos] as bit patterns, on the device."""
    import torch
    g = _plain(11, 1024, 16)
    B = 2051
    assert B * g.K > SOFT_LANES and B * g.K < SOFT_LANES + 4 * g.K            # (three rows and a bit into the second trip)
    pos = torch.from_numpy(g.systematic_positions()[0].astype(np.int64)).cuda()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    llr = torch.randn((B, g.N), generator=gen, device="cuda", dtype=torch.float64) * 7
    ext = torch.randn((B, g.N), generator=gen, device="cuda", dtype=torch.float64) * 3
    ext[torch.rand((B, g.N), generator=gen, device="cuda") < 0.1] = float("inf")
    out = torch.full((B + 2, g.K), -7.5, dtype=torch.float64, device="cuda")
    g.systematic_soft_dev(llr.data_ptr(), "f64", ext.data_ptr(), B, out[1:].data_ptr())
    g.systematic_soft_dev(llr.data_ptr(), "f64", ext.data_ptr(), B, out[1:].data_ptr())
    torch.cuda.synchronize()
    want = llr[:, pos] + ext[:, pos]
    assert bool(torch.isposinf(want).any())
    assert _first_bad_row(out[1:B + 1], want) == -1
    assert bool((out[0] == -7.5).all()) and bool((out[B + 1] == -7.5).all())
