"""The multi-level coding (MLC) receiver on the device (polar_kernels_mlc.hip) against the numpy restatement
(tests/mlc_numpy.py, bit for bit) and against the construction tables the reference ships for it
(tests/golden/construction_tables_mlc.npz, statistically)."""
import os

import numpy as np
import pytest

import mlc_numpy as R

pytestmark = pytest.mark.gpu

TABLES = np.load(os.path.join(os.path.dirname(__file__), "golden", "construction_tables_mlc.npz"))
KEYS = [str(k) for k in TABLES["keys"]]
DESIGN = {"ask4-sp": 4.5, "ask16-sp": 12.0, "ask16-gray": 13.0}


@pytest.fixture(scope="module")
def lib(built_lib):
    import polar_amd
    return polar_amd


def _handle(lib, N, K, src):
    """(handle, frozen, order): the code of a shipped table (N = 1024), or from_block_length's frozen set with a shuffled info
    order (the decoder's output order is the handle's, not the index order)."""
    if src is None:
        frozen = lib.PolarCode.from_block_length(N, K, 0.32).frozen_bits.astype(np.uint8)
        rng = np.random.default_rng(N + K)
        info = np.nonzero(frozen == 0)[0]
        order = np.concatenate([rng.permutation(info), np.nonzero(frozen)[0]]).astype(np.uint16)
    else:
        counts = TABLES[src + "/counts"].astype(np.int64)
        order = np.argsort(counts, kind="stable").astype(np.uint16)
    frozen = np.ones(N, np.uint8)
    frozen[order[:K]] = 0
    g = lib.PolarCode.from_tables(int(np.log2(N)), K, 0, frozen, order, None)
    return g, frozen, order


CASES = [("ask4-sp", 1024, "ask4-sp_4.5_250000"), ("ask16-sp", 1024, "ask16-sp_12_250000"), ("ask16-gray", 1024, None),
         ("ask4-sp", 256, None), ("ask16-sp", 256, None), ("ask4-sp", 2048, None), ("ask16-sp", 2048, None)]


@pytest.mark.parametrize("const,N,src", CASES)
def test_synth_and_decode_match_restatement(lib, const, N, src):
    import torch
    K = N // 2
    g, frozen, order = _handle(lib, N, K, src)
    cid = R.NAMES[const]
    M = N // R.nbits(cid)
    B = 40
    for snr in (DESIGN[const] - 1.0, DESIGN[const], DESIGN[const] + 1.0):
        d_y = torch.empty((B, M), dtype=torch.float64, device="cuda")
        d_i = torch.empty((B, K), dtype=torch.uint8, device="cuda")
        g.synth_mlc_dev(const, 5, 1000, B, snr, d_y.data_ptr(), d_i.data_ptr())
        torch.cuda.synchronize()
        y, info = R.synth(frozen, order, K, cid, 5, np.arange(1000, 1000 + B, dtype=np.uint64), snr)
        assert (d_y.cpu().numpy() == y).all() and (d_i.cpu().numpy() == info).all(), (const, N, snr)
        _, n0 = R.sigma_n0(snr)
        want = R.decode(frozen, order, K, y, n0, cid)
        for lat in (-1, 1 << 20):                     # lane-per-codeword kernel, one-codeword-per-wave kernel
            g.debug_set("lat_max_b", lat)
            got = g.decode_mlc(y, n0, const)
            assert np.array_equal(got, want, equal_nan=True), (const, N, snr, lat)
            assert (g.debug_get("lat_waves") > 0) == (lat > 0), (const, N, lat)       # (the forced leg did take the latency kernel)
            out = torch.empty((B, K), dtype=torch.float64, device="cuda")
            g.decode_mlc_dev(const, d_y.data_ptr(), n0, B, out.data_ptr())
            torch.cuda.synchronize()
            assert (g.debug_get("lat_waves") > 0) == (lat > 0), (const, N, lat)
            assert np.array_equal(out.cpu().numpy(), want, equal_nan=True)
        g.debug_set("lat_max_b", 0)
    # encoder, and a noiseless decode returns the info
    comps, coded = R.encode(frozen, order, K, info, cid)
    assert (g.encode_mlc(info, const) == coded).all()
    x = R.modulate(comps, cid)
    for lat in (-1, 1 << 20):
        g.debug_set("lat_max_b", lat)
        assert (g.decode_mlc(x, 1e-3, const) == info).all()
    g.debug_set("lat_max_b", 0)


def test_sweep_counters_equal_restatement(lib):
    import polar_amd
    g, frozen, order = _handle(lib, 256, 128, None)
    snr = [3.5, 4.5]
    max_runs = 600
    err, run, bit = R.sweep_counters(frozen, order, 128, R.NAMES["ask4-sp"], 3, snr, max_runs)
    assert err[0] > 0 and err[1] < err[0]                     # the skip rule: point 2 only simulates point 1's failures
    res = []
    for kw in ({}, {"devices": [0]}):
        b, ber, c = g.get_bler_quick(snr, [1], max_runs=max_runs, max_err=10 ** 9, seed=3, constellation="ask4-sp",
                                     receiver="mlc", return_ber=True, return_counters=True, **kw)
        res.append((c["err"][0].astype(np.int64), c["run"][0].astype(np.int64), ber[0]))
    b, ber, c = g.get_bler_quick_rank(snr, [1], 0, 1, lambda a: None, max_runs=max_runs, max_err=10 ** 9, seed=3,
                                      constellation="ask4-sp", receiver="mlc")
    res.append((c["err"][0].astype(np.int64), c["run"][0].astype(np.int64), ber[0]))
    for e, r, be in res:
        assert (e == err).all() and (r == run).all(), (e, err, r, run)
        assert np.allclose(be * r, bit, rtol=0, atol=1e-6), (be * r, bit)
    assert isinstance(polar_amd.RX_MLC, int)


def test_pipelined_rounds_and_montecarlo_driver_equal_restatement(lib):
    """Several rounds (batch = 128 of 600 trials): the pipelined steps merge stages of different rounds at different SNRs, each
    decoded with its own n0 at its own row offset. The trial-keyed counters do not depend on the rounds. The same sweep through
    polar_amd/montecarlo.py (one process: world = 1), and its sharded construction."""
    from polar_amd import montecarlo
    g, frozen, order = _handle(lib, 256, 128, None)
    snr = [3.0, 3.5, 4.5]
    err, run, bit = R.sweep_counters(frozen, order, 128, R.NAMES["ask4-sp"], 3, snr, 600)
    assert err[0] > err[1] > err[2] > 0
    b, ber, c = g.get_bler_quick(snr, [1], max_runs=600, max_err=10 ** 9, seed=3, batch=128, constellation="ask4-sp",
                                 receiver="mlc", return_ber=True, return_counters=True)
    assert c["rounds"] >= 5
    assert (c["err"][0].astype(np.int64) == err).all() and (c["run"][0].astype(np.int64) == run).all(), (c, err, run)
    assert np.allclose(ber[0] * run, bit, rtol=0, atol=1e-6)
    stats = {}
    b2, e2, r2 = montecarlo.get_bler_quick_ranks(g, snr, [1], max_runs=600, max_err=10 ** 9, seed=3, global_batch=128,
                                                 stats=stats, constellation="ask4-sp", receiver="mlc")
    assert (e2[0].astype(np.int64) == err).all() and (r2[0].astype(np.int64) == run).all() and stats["rounds"] >= 5
    cnt = montecarlo.mc_construction_sharded(lib.mc_construction, 8, 4.5, 64, "ask4-sp", seed=9, receiver="mlc")
    assert (cnt.astype(np.int64) == R.construction(256, R.NAMES["ask4-sp"], 4.5, 9, np.arange(64, dtype=np.uint64))).all()


def test_genie_counts_equal_restatement(lib):
    for const, snr in (("ask4-sp", 4.5), ("ask16-sp", 12.0)):
        got = lib.mc_construction(8, snr, 64, const, seed=9, trial0=17, receiver="mlc")
        want = R.construction(256, R.NAMES[const], snr, 9, np.arange(17, 17 + 64, dtype=np.uint64))
        assert (got.astype(np.int64) == want).all(), const


@pytest.mark.parametrize("key", [k for k in KEYS])
def test_every_shipped_mlc_construction_table_is_reproduced_statistically(lib, key):
    """The battery of test_construction.py's BICM table test (same thresholds) on the four MLC tables the reference ships."""
    import scipy.stats
    ref = TABLES[key + "/counts"].astype(np.float64)
    snr, runs = float(TABLES[key + "/meta"][0]), int(TABLES[key + "/meta"][1])
    const = key.split("_")[0]
    got = lib.mc_construction(10, snr, runs, const, seed=77, receiver="mlc").astype(np.float64)
    tol = 6.0 * np.sqrt(ref + got + 1.0) + 3.0
    bad = np.nonzero(np.abs(got - ref) > tol)[0]
    assert bad.size == 0, (key, bad[:10], got[bad[:10]], ref[bad[:10]])
    big = (ref + got) >= 20
    chi2 = float((((got - ref)[big] ** 2) / (got + ref)[big]).sum())
    assert big.sum() > 400 and chi2 / big.sum() < 1.25, (key, chi2, int(big.sum()))
    rho, r = scipy.stats.spearmanr(got, ref).correlation, np.corrcoef(got, ref)[0, 1]
    assert rho > 0.97 and r > 0.9999, (key, rho, r)
    assert abs(got.sum() - ref.sum()) < 3e-3 * ref.sum(), (key, got.sum(), ref.sum())
    fr_ref = np.ones(1024, np.uint8)
    fr_ref[np.argsort(ref, kind="stable")[:512]] = 0
    code = lib.PolarCode.from_counts(got, 512)
    diff = np.nonzero(code.frozen_bits != fr_ref)[0]
    thr = np.sort(ref)[511]
    assert diff.size <= 24 and (np.abs(ref[diff] - thr) < 6 * np.sqrt(thr + 1) + 10).all(), (key, diff, thr)


def test_from_monte_carlo_mlc_writes_the_reference_file_name(lib, tmp_path):
    g = lib.PolarCode.from_monte_carlo(1024, 512, 4.5, num_runs=20000, constellation_name="ask4-sp", receiver_algo="mlc",
                                       data_dir=str(tmp_path))
    names = os.listdir(tmp_path)
    assert names == ["MC_block_length_1024_512_cc_method_monte-carlo_cc_param_4.5_ask4-sp_mlc_20000.txt"], names
    g2 = lib.PolarCode.from_monte_carlo(1024, 512, 4.5, num_runs=20000, constellation_name="ask4-sp", receiver_algo="mlc",
                                        data_dir=str(tmp_path))
    assert (g.frozen_bits == g2.frozen_bits).all() and (g.construction_counts == g2.construction_counts).all()


def test_sweep_bler_within_the_reference_estimate(lib):
    """Code from the shipped ask4-sp 250 k table, 100 k sweep trials at 4.5 dB: the SC block error event is the union of the
    genie error events of the info positions, so the BLER lies between the largest info-position genie rate and (about) the
    reference's bler_estimate = sum of those rates (PolarCode.m:136)."""
    key = "ask4-sp_4.5_250000"
    counts = TABLES[key + "/counts"].astype(np.int64)
    g, frozen, order = _handle(lib, 1024, 512, key)
    rates = counts[order[:512]] / 250000.0
    b = g.get_bler_quick([4.5], [1], max_runs=100000, max_err=10 ** 9, seed=11, constellation="ask4-sp", receiver="mlc")
    assert rates.max() < b[0, 0] < 1.1 * rates.sum(), (b, rates.max(), rates.sum())


def test_refusals_leave_the_handle_usable(lib):
    import polar_amd
    g, frozen, order = _handle(lib, 256, 128, None)
    y = np.zeros((2, 128))
    with pytest.raises(polar_amd.PolarError, match="SC only"):
        g.get_bler_quick([4.0], [2], max_runs=10, constellation="ask4-sp", receiver="mlc")
    with pytest.raises(polar_amd.PolarError, match="power-of-two"):
        _handle(lib, 1024, 512, None)[0].decode_mlc(np.zeros((1, 341)), 0.1, "ask8-sp")
    with pytest.raises(polar_amd.PolarError, match="unknown constellation"):
        g.decode_mlc(y, 0.1, 9)
    # rows of any width but M = N / n_bits are refused before the library reads them
    for bad in (np.zeros((2, 100)), np.zeros((2, 256)), np.zeros(256), np.zeros((2, 2, 128))):
        with pytest.raises(polar_amd.PolarError, match=r"must be \[B\]\[128\]"):
            g.decode_mlc(bad, 0.1, "ask4-sp")
    with pytest.raises(polar_amd.PolarError, match=r"must be \[B\]\[64\]"):
        g.decode_mlc(y, 0.1, "ask16-sp")
    with pytest.raises(polar_amd.PolarError, match="power-of-two"):
        polar_amd.mc_construction(10, 9.0, 10, "ask8-sp", receiver="mlc")
    gc = polar_amd.PolarCode(8, 128, 0.32, 8)
    with pytest.raises(polar_amd.PolarError, match="no CRC"):
        gc.decode_mlc(y, 0.1, "ask4-sp")
    with pytest.raises(polar_amd.PolarError, match="no CRC"):
        gc.get_bler_quick([4.0], [1], max_runs=10, constellation="ask4-sp", receiver="mlc")
    # still usable
    x = R.modulate(R.encode(frozen, order, 128, np.zeros((1, 128), np.uint8), 5)[0], 5)
    assert (g.decode_mlc(x, 1e-3, "ask4-sp") == 0).all()
    assert (gc.decode_sc_p1(np.full(256, 0.1)) == 0).all()


def test_bicm_over_set_partition_ask16(lib):
    import torch
    g, frozen, order = _handle(lib, 1024, 512, None)
    d_llr = torch.empty((3, 1024), dtype=torch.float64, device="cuda")
    d_info = torch.empty((3, 512), dtype=torch.uint8, device="cuda")
    g.synth_bicm_llr_dev("ask16-sp", 9, 0, 3, 13.0, d_llr.data_ptr(), d_info.data_ptr())
    torch.cuda.synchronize()
    llr, info = d_llr.cpu().numpy(), d_info.cpu().numpy()
    pts = (np.arange(16) * 2 - 15) / np.sqrt(85.0)
    pts = pts / np.sqrt(np.mean(pts ** 2))
    sigma = np.sqrt(0.5) * 10 ** (-13.0 / 20)
    from test_bicm import _oracle_symbol_noise
    for t in range(3):
        coded = g.encode(info[t])
        bits = coded.reshape(-1, 4)
        y = pts[(bits * (1 << np.arange(4))).sum(1)] + _oracle_symbol_noise(9, t, 256) * sigma
        ps = np.exp(-np.abs(y[:, None] - pts[None, :]) ** 2 / 2 / sigma ** 2)
        want = np.zeros((256, 4))
        for m in range(4):
            b = (np.arange(16) >> m) & 1
            want[:, m] = np.log(ps[:, b == 0].sum(1) / ps[:, b == 1].sum(1))
        assert np.allclose(llr[t], want.reshape(-1), rtol=1e-9, atol=1e-9)
