"""The numpy restatement of the MLC receiver (tests/mlc_numpy.py) against a literal transcription of the reference's
compute_llr_mlc (Constellation.m:95-121, nested loops, libm exp) and recursive polar_decode (PolarCode.m:870-887), and the
shipped MLC construction tables' structure (tests/golden/construction_tables_mlc.npz). CPU only."""
import math
import os

import numpy as np
import pytest

import mlc_numpy as R
import mlc_rows

DESIGN = {"ask4-sp": 4.5, "ask16-sp": 12.0, "ask16-gray": 13.0}
TABLES = np.load(os.path.join(os.path.dirname(__file__), "golden", "construction_tables_mlc.npz"))


def _literal_llr_mlc(y, n0, u, cid):
    pts = R.points(cid)
    nb = R.nbits(cid)
    p0 = [0.0] * len(y)
    p1 = [0.0] * len(y)
    for yi in range(len(y)):
        for s in range(1 << nb):
            valid = True
            for m in range(len(u)):
                if float((s >> m) & 1) != u[m][yi]:
                    valid = False
            if not valid:
                continue
            m = len(u)
            # (include/polar_synth.h: polar_synth_exp_neg "flushes to 0 below 2^-1022", at x < -708, where libm goes on through
            # the denormals; the transcription takes that one rule over. Only symbols of the `loud` rows get there.)
            x = -abs(y[yi] - pts[s]) ** 2 / 2 / n0
            e = 0.0 if x < -708.0 else math.exp(x)
            if (s >> m) & 1 == 0:
                p0[yi] += e
            else:
                p1[yi] += e
    out = []
    for a, b in zip(p0, p1):
        out.append(b / (a + b) if a + b > 0 else float("nan"))
    return out


def _literal_decode(y, f):
    N = len(y)
    if N == 1:
        if f[0] == 0:
            t = 1 - 2 * y[0]
            x = (1 - ((t > 0) - (t < 0))) / 2
        else:
            x = 0.0
        return [x], [x]
    c = lambda a, b: a * (1 - b) + b * (1 - a)                                # noqa: E731
    v = lambda a, b: a * b / (a * b + (1 - a) * (1 - b)) if (a * b + (1 - a) * (1 - b)) != 0 else float("nan")  # noqa: E731
    u1, x1 = _literal_decode([c(a, b) for a, b in zip(y[0::2], y[1::2])], f[: N // 2])
    u2, x2 = _literal_decode([v(c(h, a), b) for h, a, b in zip(x1, y[0::2], y[1::2])], f[N // 2:])
    x = []
    for a, b in zip(x1, x2):
        x += [c(a, b), b]
    return u1 + u2, x


# the tiny component lengths the kernels special-case (M = 2: ask4-sp N = 4, ask16 N = 8; M = 4) up to N = 32: K = 1, N / 2 and N
TINY = [(c, N, K) for c, sizes in (("ask4-sp", (4, 8, 16, 32)), ("ask16-sp", (8, 16, 32)), ("ask16-gray", (8, 16, 32)))
        for N in sizes for K in (1, N // 2, N)]


@pytest.mark.parametrize("const,N,K", [pytest.param("ask4-sp", 64, 32, id="ask4-sp-64"), pytest.param("ask16-sp", 64, 32, id="ask16-sp-64")] + TINY)
def test_restatement_matches_literal_transcription(const, N, K):
    """Ordinary rows with the degenerate rows of mlc_rows among them (the first seven rows and every seventh). The `mid` rows (every
    symbol exactly 0.0) put every probability within a rounding of 0.5: their demapped values are held against the transcription
    like all others, but their DECISIONS are those of the rounding noise of libm's exp or of polar_synth_exp_neg, and are not
    compared (on the device they are the model's bit for bit, which is what the GPU tests assert)."""
    cid = R.NAMES[const]
    nb = R.nbits(cid)
    M = N // nb
    rng = np.random.default_rng(7)
    order = rng.permutation(N).astype(np.uint16)
    frozen = np.ones(N, np.uint8)
    frozen[order[:K]] = 0
    design = DESIGN[const]
    n_checked = 0
    B = 200 if N == 64 else 70
    for snr in (design - 2.0, design, design + 2.0):
        y, info = mlc_rows.rows(frozen, order, K, cid, 4, 0, B, snr, every=7)
        _, n0 = R.sigma_n0(snr)
        want = R.decode(frozen, order, K, y, n0, cid)
        mid = {r for r, k in mlc_rows.where(B, 7) if mlc_rows.EDGE_KINDS[k] == "mid"}
        for t in range(B):
            xs, us = [], []
            for k in range(nb):
                p1 = _literal_llr_mlc(list(y[t]), n0, xs, cid)
                with np.errstate(invalid="ignore", divide="ignore"):
                    got_p1 = R.demap(y[t:t + 1], n0, k, [np.array([x]) for x in xs], cid)[0]
                assert np.allclose(got_p1, p1, rtol=1e-12, atol=0, equal_nan=True)
                u, x = _literal_decode(p1, list(frozen[k * M:(k + 1) * M]))
                us += u
                xs.append(x)
            lit = np.array(us)[order[:K].astype(np.int64)]
            assert t in mid or np.array_equal(lit, want[t], equal_nan=True), (const, snr, t)
            n_checked += 1
    assert n_checked == 3 * B and len(mid) == (5 if B == 200 else 2)


@pytest.mark.parametrize("const,N", [("ask4-sp", 4), ("ask4-sp", 16), ("ask4-sp", 64), ("ask4-sp", 256), ("ask16-sp", 8),
                                     ("ask16-sp", 32), ("ask16-sp", 128), ("ask16-sp", 256), ("ask16-gray", 8), ("ask16-gray", 32),
                                     ("ask16-gray", 128), ("ask16-gray", 256)])
def test_degenerate_rows_are_what_they_are_for(const, N):
    """The classes of mlc_rows.EDGE_KINDS at the design n0 and at 6 dB, with warnings as errors: the model takes every row without
    one; a row with one symbol whose demapper is 0 / 0 or NaN (far, nan, inf, all_far) decides 0.5 on every unfrozen leaf; every
    symbol exactly 0.0 (mid) mixes 0, 0.5 and 1 for ask16-gray; the row x 6 (loud) puts exact 0.0 / 1.0 (16-ASK: also 0 / 0) into the level-0
    probabilities at the design n0 from 64 symbols a row on (the shorter rows are too few draws: the count is printed), next to values strictly between; the noiseless row returns the info at the design n0 (at 6 dB 16-ASK is undecided even
    without noise)."""
    import warnings
    cid = R.NAMES[const]
    K = N // 2
    frozen, order = mlc_rows.bec_code(N, K)
    kinds = mlc_rows.EDGE_KINDS
    seen_mid = set()
    for snr in (DESIGN[const], 6.0):
        _, n0 = R.sigma_n0(snr)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            y, info = mlc_rows.rows(frozen, order, K, cid, 21, 0, 16, snr)
            got = R.decode(frozen, order, K, y, n0, cid)
            with np.errstate(invalid="ignore", divide="ignore"):
                p_loud = R.demap(y[kinds.index("loud")][None, :], n0, 0, [], cid)[0]
        for kind in ("far", "nan", "inf", "all_far"):
            assert (got[kinds.index(kind)] == 0.5).all(), (kind, snr)
        seen_mid |= set(got[kinds.index("mid")].tolist())
        exact = int(((p_loud == 0.0) | (p_loud == 1.0) | np.isnan(p_loud)).sum())
        print(const, N, snr, "exact 0 / 1 or NaN in the loud row's level-0 probabilities:", exact, "of", p_loud.size)
        assert (exact >= 1 or p_loud.size < 64 or snr != DESIGN[const]) and (exact < p_loud.size or p_loud.size < 64), (snr, p_loud)       # (16-ASK: a symbol past every point by more than 708 n0 is 0 / 0, too)
        assert snr != DESIGN[const] or (got[kinds.index("clean")] == info[kinds.index("clean")]).all(), snr
    assert seen_mid == {0.0, 0.5, 1.0} if (const, N) == ("ask16-gray", 256) else seen_mid <= {0.0, 0.5, 1.0}, seen_mid


@pytest.mark.parametrize("const", ["ask4-sp", "ask8-sp", "ask16-sp", "ask16-gray"])
def test_noiseless_round_trip(const):
    cid = R.NAMES[const]
    N = 192 if const == "ask8-sp" else 256
    K = N // 2
    rng = np.random.default_rng(3)
    order = rng.permutation(N).astype(np.uint16)
    frozen = np.ones(N, np.uint8)
    frozen[order[:K]] = 0
    info = rng.integers(0, 2, (16, K)).astype(np.uint8)
    comps, coded = R.encode(frozen, order, K, info, cid)
    nb = R.nbits(cid)
    assert (coded.reshape(16, -1, nb)[:, :, 1] == comps[1]).all()
    got = R.decode(frozen, order, K, R.modulate(comps, cid), 1e-3, cid)
    assert (got == info).all()


def test_set_partition_points():
    for cid, ns in ((5, 4), (6, 8), (7, 16)):
        p = R.points(cid)
        assert (np.diff(p) > 0).all() and abs(np.mean(p ** 2) - 1) < 1e-15 and len(p) == ns


def test_shipped_tables_are_layer_major_lsb_weakest():
    keys = [str(k) for k in TABLES["keys"]]
    assert len(keys) == 4
    for k in keys:
        c = TABLES[k + "/counts"].astype(np.int64)
        assert c.shape == (1024,)
        nb = 2 if k.startswith("ask4") else 4
        M = 1024 // nb
        sums = [int(c[i * M:(i + 1) * M].sum()) for i in range(nb)]
        assert all(a > b for a, b in zip(sums, sums[1:])), (k, sums)      # layer 1 (label LSB) weakest
        info = np.argsort(c, kind="stable")[:512]
        per = [int(((info >= i * M) & (info < (i + 1) * M)).sum()) for i in range(nb)]
        assert all(a <= b for a, b in zip(per, per[1:])), (k, per)
    c = TABLES["ask16-sp_12_250000/counts"].astype(np.int64)
    assert np.sort(c, kind="stable")[:512].sum() / 250000 == pytest.approx(0.00589, abs=5e-6)
    c = TABLES["ask4-sp_4.5_250000/counts"].astype(np.int64)
    assert np.sort(c, kind="stable")[:512].sum() / 250000 == pytest.approx(0.01628, abs=5e-6)


def test_generator_port_matches_test_bicm():
    from test_bicm import _oracle_symbol_noise, _philox
    for c in ([0, 5, 0, 2], [7, 123456, 3, 1], [0xFFFFFFFF, 1, 0xABCDEF, 3]):
        want = _philox(c, [77, 1])
        got = R.philox(*[np.uint64(v) for v in c], 77, 1)
        assert [int(x) for x in got] == want
    z = R.symbol_noise(9, np.array([3], np.uint64), 64)[0]
    assert np.allclose(z, _oracle_symbol_noise(9, 3, 64), rtol=1e-13, atol=1e-13)
