"""GPU suite: the later trips of the kernels that keep one codeword (or one group) per LANE and all decoder state in a per-wave
HBM scratch — scl_decode_p1_kernel and sc_p1_kernel (polar_kernels_p1.hip), mlc_sc_kernel and mlc_genie_kernel
(polar_kernels_mlc.hip), mc_genie_kernel (polar_construct.hip). Every trip of their grid-stride loop reuses that scratch without
clearing it: layers, partial sums, history words, the re-encoded lower levels of the MLC receiver are the previous codeword's
when the next one starts. tests/test_gpu_lat_rounds.py is the same question for the one-codeword-per-wave kernels and their LDS.

Two hooks of include/polar_amd_debug.h make the trips a statement: "lane_grid" caps the blocks of the three launches that are
sized through grid_that_fits (a few hundred rows then drive a wave through three or four codewords at any block length, whatever
the CU count), and "lane_waves" tells how many blocks the last call launched. Every forced call asserts which kernel ran. The
genie kernels are launched without a handle: their second trip is reached through the public `batch` argument, with more than
8192 x 64 runs in one batch.

Also here: the component lengths M = 2 and M = 4 of the MLC receiver, where both of its decoders and its front kernel have
branches of their own, and the degenerate symbol rows of mlc_rows among all MLC inputs.

Every comparison is equality — bits and counts against the oracle, doubles against the numpy model (NaN positions apart:
p1_rows.rows_that_differ). Every reference is computed on the CPU; no kernel is held against another."""
import contextlib

import numpy as np
import pytest

import mlc_numpy as R
import mlc_rows
import p1_rows

pytestmark = pytest.mark.gpu

DESIGN = {"ask4-sp": 4.5, "ask16-sp": 12.0, "ask16-gray": 13.0}
KNOBS = ("lat_max_b", "lat_grid", "lane_grid")
LAT = 1 << 20
TINY = [("ask4-sp", N) for N in (4, 8, 16, 32, 64)] + [(c, N) for c in ("ask16-sp", "ask16-gray") for N in (8, 16, 32, 64, 128)]


@pytest.fixture(scope="module")
def lib(built_lib):
    import polar_amd
    return polar_amd


@contextlib.contextmanager
def _forced(g, **knobs):
    """The knobs for the duration of the block, every knob back at its default afterwards."""
    try:
        for k, v in knobs.items():
            g.debug_set(k, v)
        yield
    finally:
        for k in KNOBS:
            g.debug_set(k, 0)


def _ran(g, lane=0, lat=0):
    """Which kernel the last call took: `lane` blocks of the lane-per-codeword launch and no latency launch, or the reverse."""
    got = (g.debug_get("lane_waves"), g.debug_get("lat_waves"))
    assert got == (lane, lat), f"(lane_waves, lat_waves) = {got}, expected {(lane, lat)}"


def _handle(lib, N, K):
    from test_gpu_mlc import _handle as h
    return h(lib, N, K, None)


def _same(got, want, what):
    bad = p1_rows.rows_that_differ(got, want)
    assert bad.size == 0, f"{bad.size}/{want.shape[0]} rows differ from the model (first {bad[:8]}) {what}"


def _decode_both_ways(g, const, y, n0, want, what, **ran):
    """decode_mlc and decode_mlc_dev on the rows y against the model's doubles, each with the statement of what ran."""
    import torch
    B, K = want.shape
    _same(g.decode_mlc(y, n0, const), want, ("host",) + what)
    _ran(g, **ran)
    d_y = torch.from_numpy(np.array(y)).cuda()
    out = torch.full((B, K), -7.0, dtype=torch.float64, device="cuda")
    g.decode_mlc_dev(const, d_y.data_ptr(), n0, B, out.data_ptr())
    torch.cuda.synchronize()
    _ran(g, **ran)
    _same(out.cpu().numpy(), want, ("dev",) + what)


# ---- (a) mlc_sc_kernel under the cap --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("below", [0.0, 1.0])
@pytest.mark.parametrize("const", ["ask4-sp", "ask16-sp", "ask16-gray"])
def test_mlc_lane_kernel_four_trips_on_two_blocks(lib, const, below):
    """N = 256, 421 rows on two blocks: four trips, the last one ragged and with block 1 idle. Rows r and r + 128 share a lane; the
    degenerate rows sit on the first seven rows and every seventh, and 128 is no multiple of 7: degenerate and ordinary rows
    follow each other in both orders in the same lane. At the design SNR and 1 dB below lower levels decide wrongly, so the
    re-encoded levels (gc) differ from row to row and a stale one changes the demapper's input."""
    N, K, B = 256, 128, 2 * 64 * 3 + 37
    g, frozen, order = _handle(lib, N, K)
    cid = R.NAMES[const]
    snr = DESIGN[const] - below
    y, info = mlc_rows.rows(frozen, order, K, cid, 5, 1000, B, snr, every=7)
    _, n0 = R.sigma_n0(snr)
    want = R.decode(frozen, order, K, y, n0, cid)
    ordinary = np.ones(B, bool)
    ordinary[[r for r, _ in mlc_rows.where(B, 7)]] = False
    wrong = int((want[ordinary] != info[ordinary]).any(axis=1).sum())
    print(f"{const} {snr} dB: the model decodes {wrong} of {int(ordinary.sum())} ordinary rows wrongly")
    assert 0 < wrong < int(ordinary.sum())
    with _forced(g, lane_grid=2, lat_max_b=-1):
        _decode_both_ways(g, const, y, n0, want, (const, snr), lane=2)


def test_mlc_sweep_under_the_cap(lib):
    """get_bler_quick's MLC legs through mlc_decode_launch with byte output: 600 trials in rounds of 421 on two blocks."""
    g, frozen, order = _handle(lib, 256, 128)
    snr = [3.5, 4.5]
    err, run, bit = R.sweep_counters(frozen, order, 128, R.NAMES["ask4-sp"], 3, snr, 600)
    assert err[0] > err[1] > 0
    with _forced(g, lane_grid=2, lat_max_b=-1):
        b, ber, c = g.get_bler_quick(snr, [1], max_runs=600, max_err=10 ** 9, seed=3, batch=421, constellation="ask4-sp",
                                     receiver="mlc", return_ber=True, return_counters=True)
        lane, lat = g.debug_get("lane_waves"), g.debug_get("lat_waves")
    assert lat == 0 and 1 <= lane <= 2, (lane, lat)          # (the last launch of the sweep: a stage of what still failed)
    assert (c["err"][0].astype(np.int64) == err).all() and (c["run"][0].astype(np.int64) == run).all(), (c, err, run)
    assert (np.rint(ber[0] * run).astype(np.int64) == bit).all() and np.abs(ber[0] * run - bit).max() < 1e-6, (ber[0] * run, bit)


# ---- (b) mlc_sc_kernel at the real grid -----------------------------------------------------------------------------------------
def test_mlc_lane_kernel_full_and_ragged_waves(lib):
    """N = 64 ask4-sp at the grid a caller gets: one lane, a wave short of one lane, a full wave, one lane more, several blocks."""
    g, frozen, order = _handle(lib, 64, 32)
    cid = R.NAMES["ask4-sp"]
    y, _ = mlc_rows.rows(frozen, order, 32, cid, 6, 0, 200, 4.5, every=7)
    _, n0 = R.sigma_n0(4.5)
    want = R.decode(frozen, order, 32, y, n0, cid)
    with _forced(g, lat_max_b=-1):
        for B in (1, 63, 64, 65, 129, 200):
            _decode_both_ways(g, "ask4-sp", y[:B], n0, want[:B], (B,), lane=(B + 63) // 64)


# ---- (c) tiny component lengths, both kernels -----------------------------------------------------------------------------------
@pytest.mark.parametrize("const,N", TINY)
def test_mlc_tiny_block_lengths(lib, const, N):
    """Components of M = 2 (mlc_sc_lat_kernel: n == 1, the leaf read from ly[1], the left decision in lxl[1], the root from the two
    leaf decisions), M = 4 (no partial-sum walk) and on, with one unfrozen leaf, half of them and nothing frozen. 70 rows at 6 dB
    with the degenerate rows among them: a ragged second wave of the lane kernel; the latency kernel on three blocks decodes 23 or
    24 rows per wave in turn, so what its LDS holds of a row (lxl[1] and the leaf decisions at M = 2) meets the next one. The
    front kernel at N < 32 (its mask, its shift by m - 1), the encoder and the noiseless round trip at the same sizes."""
    import torch
    cid = R.NAMES[const]
    nb = R.nbits(cid)
    M, B = N // nb, 70
    _, n0 = R.sigma_n0(6.0)
    for K in (1, N // 2, N):
        g, frozen, order = _handle(lib, N, K)
        y, info = mlc_rows.rows(frozen, order, K, cid, 8, 300, B, 6.0, every=7)
        want = R.decode(frozen, order, K, y, n0, cid)
        with _forced(g, lat_max_b=-1):
            _decode_both_ways(g, const, y, n0, want, (const, N, K, "lane"), lane=2)
        with _forced(g, lat_max_b=LAT, lat_grid=3):
            _decode_both_ways(g, const, y, n0, want, (const, N, K, "lat"), lat=3)
        # the synthetic workload and the encoder
        d_y = torch.empty((B, M), dtype=torch.float64, device="cuda")
        d_i = torch.empty((B, K), dtype=torch.uint8, device="cuda")
        g.synth_mlc_dev(const, 8, 300, B, 6.0, d_y.data_ptr(), d_i.data_ptr())
        torch.cuda.synchronize()
        ys, infos = R.synth(frozen, order, K, cid, 8, np.arange(300, 300 + B, dtype=np.uint64), 6.0)
        assert (d_y.cpu().numpy() == ys).all() and (d_i.cpu().numpy() == infos).all(), (const, N, K)
        comps, coded = R.encode(frozen, order, K, infos, cid)
        assert (g.encode_mlc(infos, const) == coded).all(), (const, N, K)
        # noiseless: the info comes back, from both kernels
        x = R.modulate(comps, cid)
        for knobs, ran in (({"lat_max_b": -1}, {"lane": 2}), ({"lat_max_b": LAT, "lat_grid": 3}, {"lat": 3})):
            with _forced(g, **knobs):
                got = g.decode_mlc(x, 1e-3, const)
                _ran(g, **ran)
            assert (got == infos).all(), (const, N, K, knobs)


@pytest.mark.parametrize("n,const,snr", [(2, "ask4-sp", 4.5), (3, "ask16-sp", 12.0)])
def test_mlc_construction_of_two_symbol_components(lib, n, const, snr):
    """mlc_genie_kernel and mlc_front_kernel (mode 1: N < 32 message bits of one masked word) at M = 2: 130 runs, three waves."""
    got = lib.mc_construction(n, snr, 130, const, seed=9, trial0=17, receiver="mlc")
    want = R.construction(1 << n, R.NAMES[const], snr, 9, np.arange(17, 17 + 130, dtype=np.uint64))
    assert (got.astype(np.int64) == want).all(), (got, want)
    assert 0 < want.sum() < 130 * (1 << n)


# ---- (d) the genie kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("const", ["ask4-sp", "ask16-sp"])
def test_mlc_genie_ragged_and_batched(lib, const):
    """200 runs: three full waves and a ragged one; then the same runs in batches of 37 (a ragged wave each, several batches through
    one scratch) and of 64, accumulated through out=."""
    snr, cid = DESIGN[const], R.NAMES[const]
    want = R.construction(256, cid, snr, 9, np.arange(17, 17 + 200, dtype=np.uint64))
    got = lib.mc_construction(8, snr, 200, const, seed=9, trial0=17, receiver="mlc")
    assert (got.astype(np.int64) == want).all(), const
    acc = np.zeros(256, np.uint64)
    lib.mc_construction(8, snr, 100, const, seed=9, trial0=17, batch=37, out=acc, receiver="mlc")
    lib.mc_construction(8, snr, 100, const, seed=9, trial0=117, batch=64, out=acc, receiver="mlc")
    assert (acc.astype(np.int64) == want).all(), const


RUNS_2ND = 8192 * 64 + 70          # one batch of these: 8192 blocks, and blocks 0 and 1 go round their c0 loop a second time


@pytest.mark.parametrize("const,snr", [("bpsk", 1.0), ("ask8-gray", 9.0)])
def test_genie_second_trip(lib, oracle_built, const, snr):
    """mc_genie_kernel's second trip (and mc_front_kernel past its 8192 blocks) at N = 8. With three-bit labels two tail
    positions of the row take p1 = 0.5."""
    import oracle_lib
    got = lib.mc_construction(3, snr, RUNS_2ND, const, seed=31, trial0=5, batch=RUNS_2ND)
    want = oracle_lib.mc_construction(3, R.NAMES[const], snr, 31, 5, RUNS_2ND)
    assert (got == want).all(), (got, want)
    assert (want > 0).all() and (want < RUNS_2ND).all()


def test_mlc_genie_second_trip(lib):
    """mlc_genie_kernel's second trip and mlc_front_kernel (mode 1) past its 8192 blocks: N = 8 ask4-sp, components of M = 4."""
    got = lib.mc_construction(3, 4.5, RUNS_2ND, "ask4-sp", seed=31, trial0=5, batch=RUNS_2ND, receiver="mlc")
    trials = np.arange(5, 5 + RUNS_2ND, dtype=np.uint64)
    want = sum(R.construction(8, R.NAMES["ask4-sp"], 4.5, 31, t) for t in np.array_split(trials, 8))
    assert (got.astype(np.int64) == want).all(), (got, want)
    assert (want > 0).all()


def test_mlc_front_kernel_past_its_grid(lib):
    """mlc_front_kernel mode 0 with more rows than its 8192 blocks: the first 70 blocks make a second row in the same LDS."""
    import torch
    N, K, B = 16, 8, 8192 + 70
    g, frozen, order = _handle(lib, N, K)
    d_y = torch.empty((B, N // 2), dtype=torch.float64, device="cuda")
    d_i = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    g.synth_mlc_dev("ask4-sp", 12, 40, B, 4.5, d_y.data_ptr(), d_i.data_ptr())
    torch.cuda.synchronize()
    y, info = R.synth(frozen, order, K, R.NAMES["ask4-sp"], 12, np.arange(40, 40 + B, dtype=np.uint64), 4.5)
    assert (d_i.cpu().numpy() == info).all()
    assert (d_y.cpu().numpy() == y).all()


# ---- (f) the two probability-domain kernels under the cap -------------------------------------------------------------------------
_pairs = {}


def _pair(n, K, crc):
    if (n, K, crc) not in _pairs:
        _pairs[(n, K, crc)] = p1_rows.pair(n, K, crc)
    return _pairs[(n, K, crc)]


@pytest.mark.parametrize("L", [1, 4, 32, 64])
@pytest.mark.parametrize("n,K,crc", [(7, 64, 8), (9, 256, 8)])
def test_scl_p1_later_trips(lib, oracle_built, n, K, crc, L):
    """N = 128 and 512: the partial sums live in the HBM words g_cl / g_cr, the history in its own words, and both blocks go
    through three or more groups of codewords (64, 16, 2 and 1 codewords per wave). A degenerate row every seventh."""
    o, g = _pair(n, K, crc)
    G = 64 // L
    B = max(6 * G + 1, 40)
    p1, p0 = p1_rows.rows(o, B, 1.0, every=7)
    want = np.stack([o.decode_scl_p1(p1[i], p0[i], L) for i in range(B)])
    with _forced(g, lane_grid=2):
        got = g.decode_scl_p1(p1, p0, L)
        _ran(g, lane=2)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size}/{B} rows differ from the oracle (first {bad[:8]}) {(n, K, crc, L)}"


@pytest.mark.parametrize("n", [3, 6, 9])
def test_sc_p1_later_trips(lib, oracle_built, n):
    """325 rows on two blocks: three trips, the last ragged and with block 1 idle, at sizes that take the generic partial-sum
    walk (n = 2, where the older test reaches a second trip, takes none)."""
    N = 1 << n
    o, g = _pair(n, N // 2, 0)
    p1, _ = p1_rows.rows(o, 325, 1.0, every=7)
    want = np.stack([o.decode_sc_p1(p1[i]) for i in range(325)])
    with _forced(g, lane_grid=2, lat_max_b=-1):
        got = g.decode_sc_p1(p1)
        _ran(g, lane=2)
    bad = p1_rows.rows_that_differ(got, want)
    assert bad.size == 0, f"{bad.size}/325 rows differ from the oracle (first {bad[:8]}) n={n}"
