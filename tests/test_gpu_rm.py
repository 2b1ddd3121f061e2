"""Rate matching on the device (polar_rate_match_batch[_dev], polar_rate_recover_batch[_dev], polar_decode_scl_llr_rm_batch[_dev],
polar_synth_rm_llr_dev, polar_mc_batch_rm, polar_ga_construction_init) against the numpy restatement of
tests/rm_numpy.py and the CPU oracle: the decode of rate-matched rows equals the oracle's decode of the mirror's recovered rows on
EVERY row. The shapes are the smallest at which each mechanism can go wrong: N = 32 (a block holds several rows), an odd E with one
doubled position, N = 128 with NR's scattered pattern on both branches of its bit selection, N = 1024 (rows longer than a block's
worth of positions), N = 2048 once."""
import ctypes as C
import warnings

import numpy as np
import pytest

import rm_numpy as M
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu
PHI_DX = 1e-4
SEED = 11
BATCHES = (0, 1, 3, 65, 1000)
# (n, K, crc, E, scheme, design Eb/N0) -> the Eb/N0 per list size at which the CPU oracle fails on 10 .. 20 of the workload's trials
# 0 .. 63 at seed 11 (a BLER of 0.16 .. 0.31; chosen on the CPU with the design of tests/rm_numpy.py at phi_dx = 1e-4).
# NR at E = 100: the bit selection punctures up to Kp = 43 (Kp / E <= 7 / 16) and shortens above; Kp = 40, 48 and 64 are here.
SHAPES = {
    (5, 8, 8, 24, "puncture", 2.0): {1: 3.75, 2: 3.0, 8: 2.0, 32: 1.25},
    (5, 8, 8, 24, "shorten", 2.0): {1: 3.75, 2: 2.5, 8: 1.75, 32: 0.25},
    (5, 8, 8, 40, "repeat", 2.0): {1: 3.5, 2: 3.25, 8: 1.75, 32: 0.5},
    (5, 8, 8, 33, "repeat", 2.0): {1: 3.5, 2: 2.75, 8: 1.75, 32: 0.75},
    (7, 48, 8, 100, "puncture", 2.0): {1: 2.25, 2: 1.75, 8: 1.25, 32: 0.75},
    (7, 48, 8, 100, "shorten", 2.0): {1: 2.25, 2: 1.5, 8: 1.25, 32: 0.75},
    (7, 32, 8, 100, "nr", 2.0): {1: 2.0, 2: 1.5, 8: 0.75, 32: 0.25},
    (7, 40, 8, 100, "nr", 2.0): {1: 2.25, 2: 1.75, 8: 1.0, 32: 0.5},
    (7, 56, 8, 100, "nr", 2.0): {1: 2.5, 2: 2.0, 8: 1.5, 32: 1.0},
    (7, 56, 8, 150, "nr", 2.0): {1: 1.75, 2: 1.25, 8: 1.0, 32: 0.5},
    (7, 56, 8, 200, "repeat", 2.0): {1: 2.25, 2: 2.0, 8: 1.25, 32: 0.75},
    (10, 384, 16, 800, "puncture", 1.5): {1: 2.0, 2: 1.5, 8: 1.0, 32: 1.0},
    (10, 384, 16, 800, "shorten", 1.5): {1: 1.75, 2: 1.5, 8: 1.25, 32: 1.0},
    (11, 768, 16, 1536, "shorten", 1.5): {32: 1.0},
}
KEYS = list(SHAPES)
SMALL = [k for k in KEYS if k[0] <= 7]
_cache = {}


@pytest.fixture(scope="module")
def tables(built_lib):
    import polar_amd
    return polar_amd.ga_phi_tables(PHI_DX)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return M.build_shim(tmp_path_factory.mktemp("rm_shim"))


def _setup(key, tables):
    """(device code, mirror design, oracle) of a shape, built once."""
    if key not in _cache:
        import polar_amd
        n, K, crc, E, scheme, ebno = key
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            g = polar_amd.PolarCode.from_gauss_approx_rm(1 << n, K, E, scheme, ebno, crc, phi_dx=PHI_DX)
        d = M.design(n, K, crc, E, scheme, ebno, *tables)
        o = Oracle(n, K, 0.32, crc, srand=1)
        o.set_tables(d["frozen"], d["order"])
        o.set_crc_matrix(g.crc_matrix)
        _cache[key] = (g, d, o)
    return _cache[key]


def _workload(key, d, o, shim, ebno, trials):
    """(rx [B, E], info [B, K], s) of the given trials, from the oracle's info bits, its encoder and the shim's noise."""
    n, K, crc, E = key[:4]
    s = M.snr_sqrt_linear_rm(K, E, ebno)
    info = o.synth_llr_trials(SEED, trials, s)[1]
    coded = np.stack([o.encode(i) for i in info])
    return shim(SEED, trials, s, coded[:, d["sel"]]), info, s


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    """Equal as 64-bit patterns; a NaN (inf - inf of a repeated position: its sign is the adder's) equals any NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


# ---- construction ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_design_equals_the_mirror(built_lib, tables, key):
    g, d, _ = _setup(key, tables)
    n, K, crc, E, scheme, _ = key
    assert g.weak_leaves == 0
    assert (_bits64(g.channels) == _bits64(d["channels"])).all()
    assert (g.channel_order_descending == d["order"]).all()
    assert (g.frozen_bits == d["frozen"]).all()
    assert (g.frozen_bits[d["forced"] != 0] == 1).all()
    # (the sum runs in the device's order in the mirror too; the terms are erfc of the device and of libm: the GA tests' bound.
    # Measured on one MI355X: equal as a bit pattern on 11 of the 14 shapes, one ulp apart on (7, 48 + 8, 100) puncture
    # (0.6938501975749023 against 0.6938501975749024) and shorten, two on (7, 56 + 8, 100) NR (0.7868733758554591 against ...589))
    print("bler_estimate", g.bler_estimate, d["bler"], g.bler_estimate == d["bler"])
    np.testing.assert_allclose(g.bler_estimate, d["bler"], rtol=1e-12, atol=0)
    sel, known, short = g.rate_match_info()
    assert (sel == d["sel"]).all() and (known == d["known"]).all() and short == 1000.0


def test_construction_init_without_forced_equals_ga_construction(built_lib):
    """A constant start vector and no forced leaves: the outputs of polar_ga_construction for BPSK at the same mean LLR, bit for bit."""
    import polar_amd
    for n in (5, 9):
        cap = np.array([[0.5]])
        ch, order, pre = polar_amd.ga_construction(n, [0.0], "bpsk", "bicm", PHI_DX, 1, cap)
        mean = float(np.ravel(polar_amd.ga_mean_llr(cap))[0])
        ch2, order2, pre2 = polar_amd.ga_construction_init(n, np.full((1, 1 << n), mean), None, PHI_DX)
        assert (_bits64(ch) == _bits64(ch2)).all() and (order == order2).all() and (_bits64(pre) == _bits64(pre2)).all()


# ---- select / recover --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_rate_match_selects(built_lib, tables, key):
    import torch
    g, d, _ = _setup(key, tables)
    N, E = g.N, key[3]
    for B in BATCHES if key[0] <= 7 else (1, 65):
        coded = np.random.default_rng(B + 1).integers(0, 2, (B, N)).astype(np.uint8)
        assert (g.rate_match(coded) == coded[:, d["sel"]]).all()
        if B:
            buf = torch.full((B + 2, E), 0xA5, dtype=torch.uint8, device="cuda")
            g.rate_match_dev(_dev(coded).data_ptr(), B, buf[1:].data_ptr())
            g.rate_match_dev(_dev(coded).data_ptr(), B, buf[1:].data_ptr())
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            assert (got[1:B + 1] == coded[:, d["sel"]]).all() and (got[0] == 0xA5).all() and (got[B + 1] == 0xA5).all()


def _rx_values(seed, B, E, fmt):
    """Received rows of `fmt` with -0.0, +-inf and values of every magnitude among them; bf16 / f16 as uint16 patterns."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((B, E)) * 10.0 ** rng.integers(-3, 3, (B, E))
    flat = v.reshape(-1)
    if flat.size:
        flat[rng.integers(0, flat.size, max(1, flat.size // 7))] = -0.0
        flat[rng.integers(0, flat.size, max(1, flat.size // 11))] = np.inf
        flat[rng.integers(0, flat.size, max(1, flat.size // 13))] = -np.inf
        flat[0] = -0.0
    if fmt == "f64":
        return v
    if fmt == "f32":
        return v.astype(np.float32)
    if fmt == "f16":
        with np.errstate(over="ignore"):
            return v.astype(np.float16).view(np.uint16)
    return (v.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


@pytest.mark.parametrize("fmt", ["f64", "f32", "f16", "bf16"])
@pytest.mark.parametrize("key", KEYS)
def test_recover_equals_the_mirror_as_bit_patterns(built_lib, tables, key, fmt):
    import torch
    g, d, _ = _setup(key, tables)
    N, E = g.N, key[3]
    for B in BATCHES if (key[0] <= 7 and fmt in ("f64", "f16")) else (3, 65):
        rx = _rx_values(B + 3, B, E, fmt)
        wide = M.widen(rx, fmt).reshape(B, E)
        with np.errstate(invalid="ignore"):
            want = M.recover(wide, d["sel"], d["known"])
        got = g.rate_recover(rx, fmt=fmt)
        assert got.shape == (B, N) and _same_bits(got, want)
        if not B:
            continue
        # device form: sentinel rows around [B][N], two calls back to back on one stream, an output that is only 8-byte aligned
        sent = np.float64(-12345.678)
        buf = torch.full(((B + 2) * N + 1,), float(sent), dtype=torch.float64, device="cuda")
        d_rx = _dev(rx)
        for off in (0, 1):
            buf.fill_(float(sent))
            out = buf[off + N: off + N + B * N]
            g.rate_recover_dev(d_rx.data_ptr(), fmt, B, out.data_ptr())
            g.rate_recover_dev(d_rx.data_ptr(), fmt, B, out.data_ptr())
            torch.cuda.synchronize()
            h = buf.cpu().numpy()
            assert _same_bits(h[off + N: off + N + B * N].reshape(B, N), want)
            assert (h[: off + N] == sent).all() and (h[off + N + B * N:] == sent).all()


def test_recover_of_a_pattern_with_many_sources(built_lib):
    """E = 8 N on N = 32, every transmit position from a random coded position: up to dozens of sources per position, some none."""
    import polar_amd
    g = polar_amd.PolarCode(5, 32, 0.32, 0)
    rng = np.random.default_rng(3)
    sel = rng.integers(0, 20, 256).astype(np.uint16)
    g.set_rate_match(sel)
    rx = _rx_values(9, 65, 256, "f64")
    with np.errstate(invalid="ignore"):
        want = M.recover(rx, sel, np.zeros(32, np.uint8))
    assert _same_bits(g.rate_recover(rx), want)


# ---- workload ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SMALL + [KEYS[-2]])
def test_synth_equals_the_shim(built_lib, tables, shim, key):
    import torch
    g, d, o = _setup(key, tables)
    E, K = key[3], key[1]
    for B, t0 in ((1, 0), (65, 95)):                       # (trials 95 .. 159 cross a refresh of the info bits)
        trials = np.arange(t0, t0 + B, dtype=np.uint64)
        rx, info, s = _workload(key, d, o, shim, 2.0, trials)
        assert s == g.snr_sqrt_linear_rm(2.0)
        d_rx = torch.full((B + 1, E), 7.0, dtype=torch.float64, device="cuda")
        d_info = torch.full((B + 1, K), 0xA5, dtype=torch.uint8, device="cuda")
        g.synth_rm_llr_dev(SEED, t0, B, s, d_rx.data_ptr(), d_info.data_ptr())
        g.synth_rm_llr_dev(SEED, t0, B, s, d_rx.data_ptr(), d_info.data_ptr())
        torch.cuda.synchronize()
        assert (_bits64(d_rx.cpu().numpy()[:B]) == _bits64(rx)).all() and (d_rx.cpu().numpy()[B] == 7.0).all()
        assert (d_info.cpu().numpy()[:B] == info).all() and (d_info.cpu().numpy()[B] == 0xA5).all()


def test_synth_with_the_identity_pattern_is_the_plain_workload(built_lib):
    import polar_amd
    import torch
    g = polar_amd.PolarCode(7, 56, 0.32, 8)
    g.set_rate_match(*polar_amd.rate_match_pattern(7, 128, "repeat"))
    s = g.snr_sqrt_linear(2.0)
    assert g.snr_sqrt_linear_rm(2.0) == s
    a = torch.zeros((65, 128), dtype=torch.float64, device="cuda")
    b = torch.zeros((65, 128), dtype=torch.float64, device="cuda")
    ia = torch.zeros((65, 56), dtype=torch.uint8, device="cuda")
    ib = torch.zeros((65, 56), dtype=torch.uint8, device="cuda")
    g.synth_rm_llr_dev(SEED, 40, 65, s, a.data_ptr(), ia.data_ptr())
    g.synth_llr_dev(SEED, 40, 65, s, b.data_ptr(), ib.data_ptr())
    torch.cuda.synchronize()
    assert (_bits64(a.cpu().numpy()) == _bits64(b.cpu().numpy())).all() and (ia.cpu().numpy() == ib.cpu().numpy()).all()


# ---- decode --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_decode_equals_the_oracle_on_every_row(built_lib, tables, shim, key):
    import torch
    g, d, o = _setup(key, tables)
    n, K, crc, E, scheme, _ = key
    plain = not (M.punctured(n, d["sel"], d["known"]).any() or d["known"].any())
    for L, ebno in SHAPES[key].items():
        trials = np.arange(64, dtype=np.uint64)
        rx, info, _ = _workload(key, d, o, shim, ebno, trials)
        llr = M.recover(rx, d["sel"], d["known"])
        want = o.decode_scl_llr(llr, L)
        errs = int((want != info).any(axis=1).sum())
        print(key, "L", L, "oracle block errors", errs, "of 64")
        assert 0.05 * 64 <= errs <= 0.5 * 64
        got = g.decode_scl_llr_rm(rx, L)
        assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0]
        # device form, with the path metric, in f32 too (the widened values are what the mirror recovers)
        d_out = torch.full((65, K), 0xA5, dtype=torch.uint8, device="cuda")
        d_pm = torch.full((65,), -1.0, dtype=torch.float64, device="cuda")
        g.decode_scl_llr_rm_dev(_dev(rx).data_ptr(), "f64", 64, L, d_out.data_ptr(), d_pm.data_ptr())
        torch.cuda.synchronize()
        fb = g.debug_fallback_rows()
        if not plain:
            assert fb is None                                  # no fallback pass ran: the LLR-domain family decoded the call
        h_out, h_pm = d_out.cpu().numpy(), d_pm.cpu().numpy()
        assert (h_out[:64] == want).all() and (h_out[64] == 0xA5).all() and h_pm[64] == -1.0
        cand, pm, crc_ok, n_active, winner = g.decode_scl_llr_list(llr, L)
        rows = np.nonzero(winner >= 0)[0]
        if plain:
            # (a repetition-only pattern takes the handle's own choice: the list output's metric is the LLR-domain family's, which
            # the exp-domain kernels match to rounding; in mode 1 the call's metric is that one bit for bit)
            np.testing.assert_allclose(h_pm[rows], pm[rows, winner[rows]], rtol=1e-9)
            g.set_mode(1)
            g.decode_scl_llr_rm_dev(_dev(rx).data_ptr(), "f64", 64, L, d_out.data_ptr(), d_pm.data_ptr())
            torch.cuda.synchronize()
            g.set_mode(0)
            h_out, h_pm = d_out.cpu().numpy(), d_pm.cpu().numpy()
            assert (h_out[:64] == want).all()
        assert (_bits64(h_pm[rows]) == _bits64(pm[rows, winner[rows]])).all()
        if L == 8 and n <= 7:
            rx32 = rx.astype(np.float32)
            want32 = o.decode_scl_llr(M.recover(rx32.astype(np.float64), d["sel"], d["known"]), L)
            assert (g.decode_scl_llr_rm(rx32, L) == want32).all()


def test_repetition_only_takes_the_automatic_choice(built_lib, tables, shim):
    import torch
    key = (7, 56, 8, 200, "repeat", 2.0)
    g, d, o = _setup(key, tables)
    B = 1000
    s = g.snr_sqrt_linear_rm(1.25)
    d_rx = torch.zeros((B, 200), dtype=torch.float64, device="cuda")
    g.synth_rm_llr_dev(SEED, 0, B, s, d_rx.data_ptr())
    torch.cuda.synchronize()
    rx = d_rx.cpu().numpy()
    got = g.decode_scl_llr_rm(rx, 8)
    assert (got == g.decode_scl_llr(g.rate_recover(rx), 8)).all()
    assert (got[:64] == o.decode_scl_llr(M.recover(rx[:64], d["sel"], d["known"]), 8)).all()


# ---- sweep ---------------------------------------------------------------------------------------------------------------------------------
def _compose(g, t0, T, stride, ebno, L):
    """(errors, wrong bits) of the trials {t0 + i stride} from the parts: synth -> decode_rm -> compare."""
    import torch
    E, K = g.rate_match_info()[0].size, g.K
    span = (T - 1) * stride + 1
    d_rx = torch.zeros((span, E), dtype=torch.float64, device="cuda")
    d_info = torch.zeros((span, K), dtype=torch.uint8, device="cuda")
    g.synth_rm_llr_dev(SEED, t0, span, g.snr_sqrt_linear_rm(ebno), d_rx.data_ptr(), d_info.data_ptr())
    torch.cuda.synchronize()
    rx, info = d_rx.cpu().numpy()[::stride], d_info.cpu().numpy()[::stride]
    diff = g.decode_scl_llr_rm(rx, L) != info
    return int(diff.any(axis=1).sum()), int(diff.sum())


@pytest.mark.parametrize("key", [(7, 48, 8, 100, "puncture", 2.0), (7, 56, 8, 100, "nr", 2.0), (7, 56, 8, 200, "repeat", 2.0)])
def test_mc_batch_equals_its_parts_and_the_oracle(built_lib, tables, shim, key):
    import polar_amd
    g, d, o = _setup(key, tables)
    ebno, Ls = [1.0, 2.5], [1, 8]
    enabled = np.array([[1, 0], [1, 1]], np.uint8)
    stats = np.full((2, 2, polar_amd.RM_N), 5, np.uint64)              # (ADDED to)
    t0, T, stride = 37, 150, 3
    g.mc_batch_rm(SEED, t0, T, stride, ebno, Ls, enabled, stats)
    for li in range(2):
        for ie in range(2):
            if not enabled[li, ie]:
                assert (stats[li, ie] == 5).all()
                continue
            err, bits = _compose(g, t0, T, stride, ebno[ie], Ls[li])
            assert (stats[li, ie] - 5).tolist() == [T, err, bits], (li, ie)
    # the CPU oracle on 64 trials
    stats = np.zeros((1, 1, polar_amd.RM_N), np.uint64)
    g.mc_batch_rm(SEED, 0, 64, 1, [SHAPES[key][8]], [8], [1], stats)
    rx, info, _ = _workload(key, d, o, shim, SHAPES[key][8], np.arange(64, dtype=np.uint64))
    diff = o.decode_scl_llr(M.recover(rx, d["sel"], d["known"]), 8) != info
    assert stats[0, 0].tolist() == [64, int(diff.any(axis=1).sum()), int(diff.sum())]
    g.mc_batch_rm(SEED, 0, 0, 1, [1.0], [1], [1], stats)                # T = 0 adds nothing
    assert stats[0, 0, 0] == 64


def test_rm_stats_stops_by_the_shared_rule(built_lib, tables):
    g, _, _ = _setup((7, 48, 8, 100, "shorten", 2.0), tables)
    res = g.rm_stats([0.0, 6.0], [1, 8], max_runs=700, max_err=20, seed=3, batch=100)
    st = res["stats"]
    import polar_amd
    run, err = st[:, :, polar_amd.RM_RUN], st[:, :, polar_amd.RM_ERR]
    # a cell leaves once ERR > max_err or RUN >= max_runs; rounds of 100: the low point stops early, the high one runs out
    assert (run % 100 == 0).all() and (run <= 700).all()
    assert ((err > 20) | (run == 700)).all()
    assert (run[:, 0] < 700).all() and (err[:, 0] > 20).all() and (run[:, 1] == 700).all()
    # the round before the last one had not met the rule yet
    assert (res["bler"] == err / run).all() and (res["ber"] == st[:, :, polar_amd.RM_BIT] / (run * g.K)).all()


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------------
def test_abi_errors(built_lib, tables):
    import polar_amd
    import torch
    g, d, _ = _setup((5, 8, 8, 24, "shorten", 2.0), tables)
    L = g._L
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    ptr = C.c_void_p(buf.data_ptr())
    odd = C.c_void_p(buf.data_ptr() + 1)
    E_ARG = -1
    assert L.polar_rate_match_batch_dev(g._h, None, C.c_long(1), ptr, None) == E_ARG
    assert L.polar_rate_match_batch_dev(g._h, ptr, C.c_long(-1), ptr, None) == E_ARG
    assert L.polar_rate_recover_batch_dev(g._h, ptr, C.c_int(4), C.c_long(1), ptr, None) == E_ARG
    assert L.polar_rate_recover_batch_dev(g._h, odd, C.c_int(2), C.c_long(1), ptr, None) == E_ARG
    assert L.polar_rate_recover_batch_dev(g._h, ptr, C.c_int(0), C.c_long(1), None, None) == E_ARG
    assert L.polar_rate_recover_batch_dev(None, ptr, C.c_int(0), C.c_long(1), ptr, None) == E_ARG
    assert L.polar_decode_scl_llr_rm_batch_dev(g._h, ptr, C.c_int(0), C.c_long(1), C.c_int(0), ptr, None, None) == E_ARG
    assert L.polar_decode_scl_llr_rm_batch_dev(g._h, ptr, C.c_int(0), C.c_long(1), C.c_int(65), ptr, None, None) == E_ARG
    assert L.polar_decode_scl_llr_rm_batch_dev(g._h, ptr, C.c_int(-1), C.c_long(1), C.c_int(1), ptr, None, None) == E_ARG
    assert L.polar_decode_scl_llr_rm_batch_dev(g._h, ptr, C.c_int(0), C.c_long(-2), C.c_int(1), ptr, None, None) == E_ARG
    assert L.polar_synth_rm_llr_dev(g._h, C.c_uint64(1), C.c_uint64(0), C.c_long(1), C.c_double(1.0), None, None, None) == E_ARG
    assert L.polar_synth_rm_llr_dev(g._h, C.c_uint64(1), C.c_uint64(0), C.c_long(-1), C.c_double(1.0), ptr, None, None) == E_ARG
    # B = 0 is fine and writes nothing
    assert L.polar_rate_recover_batch_dev(g._h, ptr, C.c_int(0), C.c_long(0), ptr, None) == 0
    assert L.polar_decode_scl_llr_rm_batch_dev(g._h, ptr, C.c_int(0), C.c_long(0), C.c_int(1), ptr, None, None) == 0
    stats = np.zeros(3, np.uint64)
    for args in ((SEED, 0, -1, 1, [1.0], [1], [1], stats), (SEED, 0, 4, 0, [1.0], [1], [1], stats), (SEED, 0, 4, 1, [1.0], [65], [1], stats)):
        with pytest.raises(polar_amd.PolarError):
            g.mc_batch_rm(*args)
    # without a pattern
    h = polar_amd.PolarCode(5, 8, 0.32, 8)
    assert L.polar_rate_recover_batch_dev(h._h, ptr, C.c_int(0), C.c_long(1), ptr, None) == E_ARG
    with pytest.raises(polar_amd.PolarError, match="no rate-matching pattern"):
        h.decode_scl_llr_rm(np.zeros((1, 24)), 1)
    # a mode set by the caller survives a rate-matched decode (the override is scoped to the call)
    g.set_mode(2)
    g.decode_scl_llr_rm(np.ones((3, 24)), 8)
    assert g.debug_fallback_rows() is None
    d_llr = torch.ones((1000, 32), dtype=torch.float64, device="cuda")
    d_out = torch.zeros((1000, 8), dtype=torch.uint8, device="cuda")
    g.decode_scl_llr_dev(d_llr.data_ptr(), 1000, 8, d_out.data_ptr())
    assert g.debug_fallback_rows() is not None              # (the caller's exp-domain mode is in force again)
    g.set_mode(0)
