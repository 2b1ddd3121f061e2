"""The numpy restatement of the Gaussian-approximation construction (tests/ga_numpy.py) against literal loop transcriptions
of the reference's .m functions, against the reference's own caches (tests/golden/ga_capacity.npz), and the reference driver
main_GA_CC_Comparison.m run through it on those caches. CPU only."""
import functools
import math
import os

import numpy as np
import pytest

import ga_numpy as G
import mlc_numpy as R

FIX = np.load(os.path.join(os.path.dirname(__file__), "golden", "ga_capacity.npz"))
RATES = [1 / 32, 1 / 16, 1 / 8, 1 / 4, 2 / 4, 3 / 4, 7 / 8]
DRIVER = (("ask4-gray", "bicm"), ("ask4-sp", "mlc"), ("ask16-gray", "bicm"), ("ask16-sp", "mlc"))
# snr_needed (dB) of main_GA_CC_Comparison.m from the reference's caches; the E_b/N_0 they give (snr - 10 log10(rate * nb))
# lie on the curves of the reference's results/gauss_approx.png (checked by eye: e.g. 4-ASK Gray 6.40 dB at rate 1/16,
# 16-ASK Gray 11.92 dB at rate 2, 16-ASK SP 17.21 dB at rate 3.5)
PINNED = {
    "ask4-gray": [-5.6409, -3.4422, -0.9503, 2.0026, 5.9183, 9.4416, 11.6391],
    "ask4-sp": [-5.8824, -3.7874, -1.1559, 1.8797, 5.9267, 9.4585, 11.5916],
    "ask16-gray": [-1.9621, 0.7291, 4.1652, 8.7659, 14.932, 19.9223, 22.5589],
    "ask16-sp": [-2.4915, -0.1077, 2.7358, 6.6108, 13.216, 19.451, 22.6502],
}


# ---- literal transcriptions (scalar loops, the .m files line by line) ------------------------------------------------
def colon(a, d, b):
    return [a + k * d for k in range(int(math.floor((b - a) / d + 1e-9)) + 1)]


def lit_bicm_capacity(cid, snr_db):                      # Constellation.m:250-286
    pts = list(R.points(cid))
    nb, ns = R.nbits(cid), len(pts)
    sigma = math.sqrt(1 / 2) * math.pow(10, -snr_db / 20)
    n_0 = sigma ** 2
    y_min = max(pts) + 6 * sigma + 1
    delta_y = sigma * 0.1
    y_vec = colon(-y_min, delta_y, y_min)
    cap = []
    for i_bit in range(nb):
        h_y = h_y_u = 0.0
        for y in y_vec:
            p_y, p_y_u = 0.0, [0.0, 0.0]
            for s in range(ns):
                e = math.exp(-(y - pts[s]) ** 2 / 2 / n_0) / math.sqrt(2 * math.pi * n_0) / ns
                p_y += e
                p_y_u[(s >> i_bit) & 1] += e * 2
            if p_y > 0:
                h_y += math.log2(p_y) * p_y * delta_y * (-1)
            for u in range(2):
                if p_y_u[u] > 0:
                    h_y_u += 0.5 * math.log2(p_y_u[u]) * p_y_u[u] * delta_y * (-1)
        cap.append(h_y - h_y_u)
    return np.array(cap)


def lit_mlc_capacity(cid, snr_db):                       # Constellation.m:190-248
    pts = list(R.points(cid))
    nb, ns = R.nbits(cid), len(pts)
    sigma = math.sqrt(1 / 2) * math.pow(10, -snr_db / 20)
    n_0 = sigma ** 2
    y_min = max(pts) + 6 * sigma + 1
    delta_y = sigma * 0.01
    y_vec = colon(-y_min, delta_y, y_min)
    h_y, h_y_given_u = [0.0] * nb, [0.0] * nb
    for i_bit in range(1, nb + 1):
        num_sets = 2 ** (i_bit - 1)
        for y in y_vec:
            p_y = [0.0] * num_sets
            p_y_u = [[0.0, 0.0] for _ in range(num_sets)]
            for i_sym in range(1, ns + 1):
                set_index = 1
                if i_bit > 1:
                    a = format(i_sym - 1, "0%db" % nb)
                    set_index = int(a[nb - i_bit + 1:nb], 2) + 1
                e = math.exp(-(y - pts[i_sym - 1]) ** 2 / 2 / n_0) / math.sqrt(2 * math.pi * n_0) / ns
                p_y[set_index - 1] += e
                p_y_u[set_index - 1][((i_sym - 1) >> (i_bit - 1)) & 1] += e * 2
            for q in range(num_sets):
                if p_y[q] > 0:
                    h_y[i_bit - 1] += (-math.log2(p_y[q])) * p_y[q] * delta_y
                for u in range(2):
                    if p_y_u[q][u] > 0:
                        h_y_given_u[i_bit - 1] += (-math.log2(p_y_u[q][u])) * p_y_u[q][u] * 0.5 * delta_y
    return np.array(h_y) - np.array(h_y_given_u)


def lit_bpsk_cap(snr_db):                                # get_bpsk_cap.m
    n_0 = 1 / 2 * math.pow(10, -snr_db / 10)
    delta_y = math.sqrt(n_0) * 0.001
    max_value = min(10000, 1 + 3 + 3 * math.sqrt(n_0))
    y_vec = colon(-max_value, delta_y, max_value)
    p_y = [sum(math.exp(-(y - x) ** 2 / 2 / n_0) / math.sqrt(2 * math.pi * n_0) * 0.5 for x in (-1, 1)) for y in y_vec]
    s = sum(p_y) * delta_y
    h = sum(-math.log2(p / s) * (p / s) * delta_y for p in p_y if p / s > 0)
    return h - 0.5 * (1 + math.log(2 * math.pi * n_0)) / math.log(2)


def lit_phi(x_increment):                                # initialize_phi.m (math.log for -log phi)
    fwd = []
    for x in colon(0, 0.01, 100.01):
        fwd.append(math.exp(-0.4527 * x ** 0.86 + 0.0218) if x < 10 else math.sqrt(math.pi / x) * (1 - 1.4286 / x) * math.exp(-x / 4))
    inv = [0.0] * G.PHI_INV
    for x in colon(0, x_increment, 400):
        ph = math.exp(-0.4527 * x ** 0.86 + 0.0218) if x < 10 else \
            math.sqrt(math.pi / (x + 0.0001)) * (1 - 1.4286 / (x + 0.0001)) * math.exp(-x / 4)
        mlp = -math.log(min(ph, 1))
        if mlp < 100 + 1e-3:
            idx = math.ceil(mlp / 1e-3)
            if idx < G.PHI_INV:
                inv[idx] = x                              # last write wins
    return np.array(fwd), np.array(inv)


def lit_round(v):
    return math.floor(v + 0.5) if v >= 0 else -math.floor(-v + 0.5)


def lit_polarization(llr_vec, n, fwd, inv):              # calculate_awgn_polarization.m with phi_x_table.m, phi_x_inv.m
    ch = list(llr_vec)
    for _ in range(n):
        c1, c2 = ch[0::2], ch[1::2]
        a = []
        for u, v in zip(c1, c2):
            pu = fwd[lit_round(min(max(u, 0), 100) / 0.01)]
            pv = fwd[lit_round(min(max(v, 0), 100) / 0.01)]
            y = 1 - (1 - pu) * (1 - pv)
            m = min(max(-float(R.synth_log(np.array([y]))[0]), 0), 100)
            a.append(inv[lit_round(m / 1e-3 - 0.499)])
        ch = a + [u + v for u, v in zip(c1, c2)]
    return np.array(ch)


def lit_capacity_llr(y, info):                           # PolarCode.m:931-945 polar_decode_capacity_llr -> (x, u)
    N = len(y)
    if N == 1:
        return [info[0]], [y[0]]

    def cnop_llr(a, b):
        t = math.tanh(a / 2) * math.tanh(b / 2)
        return math.copysign(math.inf, t) if abs(t) == 1 else 2 * math.atanh(t)
    u1est = [cnop_llr(a, b) for a, b in zip(y[0::2], y[1::2])]
    x1, u1 = lit_capacity_llr(u1est, info[: N // 2])
    u2est = [(1 - 2 * h) * a + b for h, a, b in zip(x1, y[0::2], y[1::2])]
    x2, u2 = lit_capacity_llr(u2est, info[N // 2:])
    x = []
    for a, b in zip(x1, x2):
        x += [a ^ b, b]
    return x, u1 + u2


# ---- restatement == transcription -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.SUPPORTED)
def test_bicm_capacity_matches_transcription(name):
    cid = R.NAMES[name]
    for snr in (-10.0, 3.25):
        np.testing.assert_allclose(G.bicm_capacity(cid, snr), lit_bicm_capacity(cid, snr), rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("name", ("bpsk", "ask4-sp", "ask4-gray"))
def test_mlc_capacity_matches_transcription(name):
    cid = R.NAMES[name]
    np.testing.assert_allclose(G.mlc_capacity(cid, -2.0), lit_mlc_capacity(cid, -2.0), rtol=1e-11, atol=1e-14)


def test_bpsk_cap_matches_transcription():
    for snr in (-20.0, -3.5):
        assert abs(G.bpsk_cap(snr) - lit_bpsk_cap(snr)) <= 1e-11 * abs(lit_bpsk_cap(snr))


def test_phi_tables_match_transcription():
    fwd, inv = lit_phi(0.01)
    f = G.phi_fwd()
    np.testing.assert_allclose(f, fwd, rtol=1e-15)
    got = G.phi_inv(0.01)
    bad = np.nonzero(got != inv)[0]
    # math.log vs the fixed-order log: an entry may move only when its x lies within 1e-12 of a bin edge
    for b in bad:
        x = max(got[b], inv[b])
        v = float(G.phi_inv_minus_log(np.array([x]))[0]) / 1e-3
        assert abs(v - round(v)) <= 1e-12 * v, (b, got[b], inv[b])
    assert bad.size <= 2


def test_mround_is_half_away_from_zero():
    v = np.array([0.5, 1.5, 2.5, -0.5, -2.5, 0.49999999999999994, 2.4999999999999996, 7.0])
    assert G.mround(v).tolist() == [1.0, 2.0, 3.0, -1.0, -3.0, 0.0, 2.0, 7.0]
    assert np.round(2.5) == 2.0                          # (numpy's own round is half to even)


def test_polarization_matches_transcription():
    fwd, inv = G.phi_fwd(), G.phi_inv(1e-3)
    for m, llr in ((1, [0.7]), (4, [1.3]), (5, [12.0]), (3, [0.05])):
        want = lit_polarization([llr[0]] * (1 << m), m, fwd, inv)
        got = G.awgn_polarization(np.full(1 << m, llr[0]), m, fwd, inv)
        assert (got == want).all()


def test_llr_for_capacity_and_bins():
    tab = FIX["bpsk_cap"][:, 1]
    # get_bpsk_llr_for_capacity.m: first entry reaching the target; none -> the last (20 dB)
    for c in (0.0, 0.3, 0.999, 1.5):
        k = next((i for i in range(len(tab)) if tab[i] >= c), len(tab) - 1)
        assert G.mean_llr([c], tab)[0] == 4 * math.pow(10.0, (-20.0 + k * 0.01) / 10)
    assert G.mean_llr([2.0], tab)[0] == 400.0
    # Constellation.m:331-341: NaN -> -100 (bin 1), clip, floor
    assert G.llr_bins(np.array([np.nan, -np.inf, np.inf, -100.0, 0.0, 0.24, 0.25, 99.99, 100.0])).tolist() == \
        [0, 0, 800, 0, 400, 400, 401, 799, 800]


def test_genie_llr_matches_transcription():
    rng = np.random.default_rng(5)
    for nb in (1, 2, 4):
        y = rng.normal(0, 6, (50, nb))
        y[0, 0], y[1, -1] = np.inf, -np.inf
        info = rng.integers(0, 2, (50, nb)).astype(np.uint8)
        x, u = G.genie_llr(y, info)
        for s in range(50):
            lx, lu = lit_capacity_llr(list(y[s]), [int(v) for v in info[s]])
            assert list(x[s]) == lx
            np.testing.assert_allclose(u[s], lu, rtol=1e-10, atol=1e-12)


def test_polarized_capacity_restatement_is_the_reference_procedure():
    # counts through the same draws as the Monte-Carlo construction's runs at N = nb; histogram entropy, min(., 1)
    cnt = G.polarized_counts(R.ASK4_GRAY, 3.0, 1, 0, 4000)
    assert cnt.shape == (2, G.BINS, 2) and int(cnt.sum()) == 2 * 4000
    cap = G.capacity_from_counts(cnt)
    assert (cap > 0).all() and (cap <= 1).all()
    # summed disjoint ranges == one range
    two = G.polarized_counts(R.ASK4_GRAY, 3.0, 1, 0, 1500) + G.polarized_counts(R.ASK4_GRAY, 3.0, 1, 1500, 2500)
    assert (two == cnt).all()


def test_rate_walk_matches_driver_loop():
    # main_GA_CC_Comparison.m:34-66 literally, on a synthetic decreasing estimate table
    snr = -10.0 + np.arange(80) * 0.25
    rng = np.random.default_rng(3)
    rates = RATES[:4]
    bler = np.exp(-np.outer(snr + 11, [3.0, 2.0, 1.5, 1.0]) + rng.normal(0, 0.01, (80, 4)))
    got, ebno, flags = G.rate_walk(bler, rates, snr, 1e-5, 2)
    start = 1
    for r in range(4):
        for si in range(start, 81):
            b = bler[si - 1, r]
            if b < 1e-5:
                break
            prev = b
        assert si != start
        start = max(si - 1, 1)
        want = (snr[si - 1] * math.log(prev / 1e-5) + snr[si - 2] * math.log(1e-5 / b)) / math.log(prev / b)
        assert got[r] == want and flags[r] == 0
        assert ebno[r] == want - 10 * math.log10(rates[r]) - 10 * math.log10(2)
    # deviations: met at the first SNR tried, and never met -> NaN with a flag
    _, _, f = G.rate_walk(np.full((80, 1), 1e-9), [0.5], snr, 1e-5, 2)
    assert f.tolist() == [1]
    s, _, f = G.rate_walk(np.full((80, 1), 1.0), [0.5], snr, 1e-5, 2)
    assert f.tolist() == [2] and np.isnan(s[0])


# ---- restatement == the reference's caches ----------------------------------------------------------------------------
def test_bpsk_cap_matches_reference_table():
    """The whole 4 001-point bpsk_cap.mat. Measured: max |diff| 6.6e-6 (at -19.85 dB: the reference's colon range and sum
    order differ from the written-down grid, and the low-SNR capacity is a difference of two entropies near 5 bits),
    2.2e-7 above -10 dB, 3.7e-13 above 0 dB. The SNR axis itself differs from -20 + k * 0.01 by at most 3.6e-15."""
    tab = FIX["bpsk_cap"]
    np.testing.assert_allclose(tab[:, 0], G.BPSK_SNR, rtol=0, atol=1e-12)
    got = np.array([G.bpsk_cap(s) for s in G.BPSK_SNR])
    d = np.abs(got - tab[:, 1])
    assert d.max() <= 7e-6
    assert d[G.BPSK_SNR > -10].max() <= 3e-7
    assert d[G.BPSK_SNR > 0].max() <= 1e-12


@functools.lru_cache(maxsize=1)
def _phi_1e5():
    return G.phi_fwd(), G.phi_inv(1e-5)


def _driver_bler(name, rx, N=1024):
    fwd, inv = _phi_1e5()
    cid = R.NAMES[name]
    nb = R.nbits(cid)
    snr = -10.0 + np.arange(161) * 0.25
    Ks = [math.ceil(r * N) for r in RATES]
    bler = np.full((161, len(RATES)), np.nan)
    for i, s in enumerate(snr):
        if rx == "mlc":
            cap = G.mlc_capacity(cid, s)
        else:
            m = (FIX["pol_const"] == name) & (FIX["pol_snr"] == s)
            if not m.any():
                continue                                  # the reference never needed this SNR
            cap = FIX["pol_cap"][m][0][:nb]
        _, _, pre = G.ga_design(N, nb, cap, FIX["bpsk_cap"][:, 1], fwd, inv)
        bler[i] = pre[[k - 1 for k in Ks]]
    return snr, bler


@pytest.mark.parametrize("name,rx", DRIVER)
def test_driver_on_reference_caches(name, rx):
    snr, bler = _driver_bler(name, rx)
    got, ebno, flags = G.rate_walk(bler, RATES, snr, 1e-5, R.nbits(R.NAMES[name]))
    assert (flags == 0).all() and np.isfinite(got).all()
    np.testing.assert_allclose(got, PINNED[name], atol=1e-4)


def test_library_rate_walk_equals_restatement():
    """polar_amd.ga_rate_table's walk (polar_amd._rate_walk) against the restatement's, which is checked against the literal
    driver loop above: same snr_needed, ebno_needed and flags, bit for bit, on shared tables (monotone, noisy, met at the
    first SNR, never met, and tables whose rates stop at adjacent indices)."""
    import polar_amd
    snr = -10.0 + np.arange(60) * 0.25
    rng = np.random.default_rng(8)
    tables = [np.exp(-np.outer(snr + 11, [3.0, 2.0, 1.5, 1.0, 0.7, 0.5, 0.45]) + rng.normal(0, s, (60, 7)))
              for s in (0.0, 0.05, 0.5)]
    tables.append(np.full((60, 7), 1e-9))
    tables.append(np.full((60, 7), 1.0))
    t = np.exp(-np.outer(snr + 11, [3.0, 3.0, 3.0, 0.2, 0.2, 5.0, 5.0]))
    tables.append(t)
    for nb in (1, 2, 4):
        for tab in tables:
            a = polar_amd._rate_walk(tab, RATES, snr, 1e-5, nb)
            b = G.rate_walk(tab, RATES, snr, 1e-5, nb)
            for x, y in zip(a, b):
                assert np.array_equal(x, y, equal_nan=True)
