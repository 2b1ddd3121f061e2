"""The numpy restatement of the MLC receiver (tests/mlc_numpy.py) against a literal transcription of the reference's
compute_llr_mlc (Constellation.m:95-121, nested loops, libm exp) and recursive polar_decode (PolarCode.m:870-887), and the
shipped MLC construction tables' structure (tests/golden/construction_tables_mlc.npz). CPU only."""
import math
import os

import numpy as np
import pytest

import mlc_numpy as R

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
            e = math.exp(-abs(y[yi] - pts[s]) ** 2 / 2 / n0)
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


@pytest.mark.parametrize("const,N", [("ask4-sp", 64), ("ask16-sp", 64)])
def test_restatement_matches_literal_transcription(const, N):
    cid = R.NAMES[const]
    nb = R.nbits(cid)
    M = N // nb
    rng = np.random.default_rng(7)
    order = rng.permutation(N).astype(np.uint16)
    K = N // 2
    frozen = np.ones(N, np.uint8)
    frozen[order[:K]] = 0
    design = {"ask4-sp": 4.5, "ask16-sp": 12.0}[const]
    n_checked = 0
    for snr in (design - 2.0, design, design + 2.0):
        y, info = R.synth(frozen, order, K, cid, 4, np.arange(200, dtype=np.uint64), snr)
        _, n0 = R.sigma_n0(snr)
        want = R.decode(frozen, order, K, y, n0, cid)
        for t in range(200):
            xs, us = [], []
            for k in range(nb):
                p1 = _literal_llr_mlc(list(y[t]), n0, xs, cid)
                got_p1 = R.demap(y[t:t + 1], n0, k, [np.array([x]) for x in xs], cid)[0]
                assert np.allclose(got_p1, p1, rtol=1e-12, atol=0, equal_nan=True)
                u, x = _literal_decode(p1, list(frozen[k * M:(k + 1) * M]))
                us += u
                xs.append(x)
            lit = np.array(us)[order[:K].astype(np.int64)]
            assert np.array_equal(lit, want[t], equal_nan=True), (const, snr, t)
            n_checked += 1
    assert n_checked == 600


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
