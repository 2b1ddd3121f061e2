"""numpy restatement of the Gaussian-approximation (GA) code construction (PolarM/PolarCode.m:198-255,
GaussianApproximation/*.m, CapacityHelper/*.m, Constellation.m:190-370, main_GA_CC_Comparison.m) as the device computes it
(polar_amd/csrc/polar_kernels_ga.hip, polar_ga.cpp).

Index rules made explicit: MATLAB `round` is half away from zero (numpy's is half to even), `ceil` as is, a NaN u-LLR lands in
bin 1 (MATLAB's max drops NaN), and the capacity-to-LLR lookup leaves its index at the last entry when nothing reaches the
target. -log(phi) goes through the fixed-order log of include/polar_synth.h (mlc_numpy.synth_log), as on the device. The
polarized-capacity draw is the Monte-Carlo construction's run at N = n_bits (mlc_numpy.philox / symbol_noise)."""
import math

import numpy as np

import mlc_numpy as R

SUPPORTED = ("bpsk", "ask4-gray", "ask4-sp", "ask16-gray", "ask16-sp")
PHI_FWD, PHI_INV, BINS = 10002, 100001, 801


def mround(v):
    """MATLAB round: half away from zero (exact: v - trunc(v) is exact in binary floating point)."""
    v = np.asarray(v, np.float64)
    t = np.trunc(v)
    return t + np.where(np.abs(v - t) >= 0.5, np.sign(v), 0.0)


def sigma(snr_db):
    return math.sqrt(1.0 / 2) * math.pow(10.0, -snr_db / 20)


def grid(n0, ymax, dy):
    """y_k = -ymax + k * dy, k = 0 .. P-1, P = floor(2 ymax / dy + 1e-9) + 1 (the reference's colon range, written down)."""
    P = int(math.floor(2 * ymax / dy + 1e-9)) + 1
    return -ymax + np.arange(P, dtype=np.float64) * dy


# ---- capacity integrals ---------------------------------------------------------------------------------------------
def bicm_capacity(cid, snr_db):
    """get_bicm_capacity (Constellation.m:250-286) -> [nb]."""
    pts = R.points(cid)
    nb, ns = R.nbits(cid), len(pts)
    s = sigma(snr_db)
    n0 = s * s
    y = grid(n0, float(pts.max()) + 6 * s + 1, s * 0.1)
    dy = s * 0.1
    c = math.sqrt(2 * math.pi * n0)
    e = [np.exp(-((y - pts[q]) * (y - pts[q])) / 2 / n0) / c / ns for q in range(ns)]
    py = np.zeros_like(y)
    for q in range(ns):
        py = py + e[q]
    hy = np.where(py > 0, np.log2(np.where(py > 0, py, 1.0)) * py * dy * (-1), 0.0).sum()
    out = np.zeros(nb)
    for b in range(nb):
        pu = [np.zeros_like(y), np.zeros_like(y)]
        for q in range(ns):
            pu[(q >> b) & 1] = pu[(q >> b) & 1] + e[q] * 2
        hu = sum(np.where(p > 0, 0.5 * np.log2(np.where(p > 0, p, 1.0)) * p * dy * (-1), 0.0) for p in pu).sum()
        out[b] = hy - hu
    return out


def mlc_capacity(cid, snr_db):
    """get_mlc_capacity (Constellation.m:190-248) -> [nb]: layer b conditioned on the label bits below it."""
    pts = R.points(cid)
    nb, ns = R.nbits(cid), len(pts)
    s = sigma(snr_db)
    n0 = s * s
    dy = s * 0.01
    y = grid(n0, float(pts.max()) + 6 * s + 1, dy)
    c = math.sqrt(2 * math.pi * n0)
    e = [np.exp(-((y - pts[q]) * (y - pts[q])) / 2 / n0) / c / ns for q in range(ns)]
    out = np.zeros(nb)
    for b in range(nb):
        hy = np.zeros_like(y)
        hu = np.zeros_like(y)
        for st in range(1 << b):
            py, pu = np.zeros_like(y), [np.zeros_like(y), np.zeros_like(y)]
            for q in range(st, ns, 1 << b):
                py = py + e[q]
                pu[(q >> b) & 1] = pu[(q >> b) & 1] + e[q] * 2
            hy = hy + np.where(py > 0, (-np.log2(np.where(py > 0, py, 1.0))) * py * dy, 0.0)
            for p in pu:
                hu = hu + np.where(p > 0, (-np.log2(np.where(p > 0, p, 1.0))) * p * 0.5 * dy, 0.0)
        out[b] = hy.sum() - hu.sum()
    return out


def bpsk_cap(snr_db):
    """get_bpsk_cap.m."""
    n0 = 1.0 / 2 * math.pow(10.0, -snr_db / 10)
    dy = math.sqrt(n0) * 0.001
    y = grid(n0, min(10000.0, 1.0 + 3 + 3 * math.sqrt(n0)), dy)
    c = math.sqrt(2 * math.pi * n0)
    py = np.zeros_like(y)
    for x in (-1.0, 1.0):
        py = py + np.exp(-((y - x) * (y - x)) / 2 / n0) / c * 0.5
    py = py / (py.sum() * dy)
    h = np.where(py > 0, (-np.log2(np.where(py > 0, py, 1.0))) * py * dy, 0.0).sum()
    return h - 0.5 * (1 + math.log(2 * math.pi * n0)) / math.log(2.0)


BPSK_SNR = -20.0 + np.arange(4001) * 0.01          # bpsk_cap.mat snr_vec_db, s_k = -20 + k * 0.01


def mean_llr(capacity, bpsk_table):
    """get_bpsk_llr_for_capacity.m: the first table entry reaching each capacity, else (no break) the last."""
    cap = np.asarray(capacity, np.float64)
    tab = np.asarray(bpsk_table, np.float64)
    out = np.empty(cap.shape)
    for i, c in np.ndenumerate(cap):
        hit = np.nonzero(tab[:-1] >= c)[0]
        k = int(hit[0]) if hit.size else len(tab) - 1
        out[i] = 4 * math.pow(10.0, (-20.0 + k * 0.01) / 10)
    return out


# ---- phi tables (initialize_phi.m) ----------------------------------------------------------------------------------
def phi_fwd():
    x = np.arange(PHI_FWD, dtype=np.float64) * 0.01
    lo = np.exp(-0.4527 * np.power(x, 0.86) + 0.0218)
    xs = np.where(x < 10, 10.0, x)
    hi = np.sqrt(math.pi / xs) * (1 - 1.4286 / xs) * np.exp(-xs / 4)
    return np.where(x < 10, lo, hi)


def phi_inv_minus_log(x):
    """-log(min(phi(x), 1)) of the inverse table's x values (the +0.0001 form)."""
    lo = np.exp(-0.4527 * np.power(x, 0.86) + 0.0218)
    xs = np.where(x < 10, 10.0, x)
    hi = np.sqrt(math.pi / (xs + 0.0001)) * (1 - 1.4286 / (xs + 0.0001)) * np.exp(-xs / 4)
    ph = np.minimum(np.where(x < 10, lo, hi), 1.0)
    return -R.synth_log(ph)


def phi_inv(dx, chunk=1 << 22):
    """Inverse table: bin ceil(-log phi / 1e-3) keeps the largest x = k * dx mapping to it (0 where none)."""
    nx = int(math.floor(400 / dx + 1e-6)) + 1
    tab = np.zeros(PHI_INV)
    for k0 in range(0, nx, chunk):
        x = np.arange(k0, min(nx, k0 + chunk), dtype=np.float64) * dx
        mlp = phi_inv_minus_log(x)
        ok = mlp < 100 + 1e-3
        b = np.ceil(mlp[ok] / 1e-3).astype(np.int64)
        keep = b < PHI_INV
        np.maximum.at(tab, b[keep], x[ok][keep])
    return tab


def phi_tab(fwd, x):
    """phi_x_table.m."""
    x = np.minimum(np.maximum(x, 0.0), 100.0)
    return fwd[mround(x / 0.01).astype(np.int64)]


def phi_x_inv(inv, y):
    """phi_x_inv.m."""
    v = -R.synth_log(y)
    v = np.minimum(np.maximum(v, 0.0), 100.0)
    return inv[mround(v / 1e-3 - 0.499).astype(np.int64)]


# ---- GA polarization ------------------------------------------------------------------------------------------------
def bitrev(m):
    M = 1 << m
    return np.array([int(format(i, "0%db" % m)[::-1], 2) if m else 0 for i in range(M)], np.int64)


def awgn_polarization(llr, m, fwd, inv):
    """calculate_awgn_polarization.m on rows [..., 2^m]."""
    ch = np.array(llr, np.float64)
    for _ in range(m):
        c1, c2 = ch[..., 0::2], ch[..., 1::2]
        ch = np.concatenate([phi_x_inv(inv, 1 - (1 - phi_tab(fwd, c1)) * (1 - phi_tab(fwd, c2))), c1 + c2], axis=-1)
    return ch


def ga_channels(N, nb, mllr, fwd, inv):
    """PolarCode.m:227-246 for mean LLRs [nb] -> channels [N]."""
    M = N // nb
    m = M.bit_length() - 1
    ch = np.empty(N)
    br = bitrev(m)
    for k in range(nb):
        tmp = awgn_polarization(np.full(M, mllr[k]), m, fwd, inv)
        ch[k * M:(k + 1) * M] = tmp[br]
    return ch


def qfunc_terms(c):
    return np.array([0.5 * math.erfc(math.sqrt(v) / 2) for v in np.asarray(c, np.float64)])


def ga_design(N, nb, capacity, bpsk_table, fwd, inv):
    """(channels, order, bler_prefix): order = stable descending sort (PolarCode.m:248), prefix sums of qfunc along it."""
    ch = ga_channels(N, nb, mean_llr(capacity, bpsk_table), fwd, inv)
    order = np.argsort(-ch, kind="stable")
    return ch, order, np.cumsum(qfunc_terms(ch[order]))


# ---- polarized capacity (Constellation.m:288-370) -------------------------------------------------------------------
def cnop_llr(a, b):
    with np.errstate(all="ignore"):
        return 2 * np.arctanh(np.tanh(a / 2) * np.tanh(b / 2))


def genie_llr(y, info):
    """polar_decode_capacity_llr (PolarCode.m:931-945) on rows [S][n] -> (x, u)."""
    n = y.shape[1]
    if n == 1:
        return info.copy(), y.copy()
    x1, u1 = genie_llr(cnop_llr(y[:, 0::2], y[:, 1::2]), info[:, : n // 2])
    with np.errstate(all="ignore"):
        x2, u2 = genie_llr((1 - 2 * x1.astype(np.float64)) * y[:, 0::2] + y[:, 1::2], info[:, n // 2:])
    x = np.empty_like(info)
    x[:, 0::2], x[:, 1::2] = x1 ^ x2, x2
    return x, np.concatenate([u1, u2], axis=1)


def genie_llr_err(y, info):
    """genie_llr plus a per-position bound on how far another correctly rounded tanh / atanh (the device's) can move each
    u-LLR: 0 where the value comes from the demapper and additions alone (bit-identical on host and device); through a
    check node, the inputs' bounds plus 4e-16 e^|out| (one ulp of tanh(.) * tanh(.) near +-1, through atanh) plus
    1e-15 |out|; inf where the check node saturates on this side (the other side may stay finite)."""
    n = y.shape[1]
    if n == 1:
        return info.copy(), y.copy(), np.zeros_like(y)
    return _genie_err(y, np.zeros_like(y), info)


def _genie_err(y, e, info):
    n = y.shape[1]
    if n == 1:
        return info.copy(), y.copy(), e.copy()
    c = cnop_llr(y[:, 0::2], y[:, 1::2])
    with np.errstate(all="ignore"):
        ce = e[:, 0::2] + e[:, 1::2] + 4e-16 * np.exp(np.minimum(np.abs(np.nan_to_num(c)), 700)) + 1e-15 * np.abs(c)
        ce = np.where(np.isfinite(c) | ~np.isfinite(y[:, 0::2]) & ~np.isfinite(y[:, 1::2]), ce, np.inf)
    x1, u1, e1 = _genie_err(c, ce, info[:, : n // 2])
    with np.errstate(all="ignore"):
        v = (1 - 2 * x1.astype(np.float64)) * y[:, 0::2] + y[:, 1::2]
        ve = e[:, 0::2] + e[:, 1::2]
        ve = ve + np.where(ve > 0, 2.3e-16 * np.abs(v), 0.0)
    x2, u2, e2 = _genie_err(v, ve, info[:, n // 2:])
    x = np.empty_like(info)
    x[:, 0::2], x[:, 1::2] = x1 ^ x2, x2
    return x, np.concatenate([u1, u2], axis=1), np.concatenate([e1, e2], axis=1)


def bicm_llr(y, n0, cid):
    """Constellation.m:123-144 with the fixed-order exp / log of polar_synth.h, [S] -> [S][nb]."""
    pts = R.points(cid)
    nb = R.nbits(cid)
    p0 = np.zeros((y.size, nb))
    p1 = np.zeros((y.size, nb))
    for s in range(len(pts)):
        d = np.abs(y - pts[s])
        ps = R.exp_neg(-(d * d) / 2 / n0)
        for m in range(nb):
            if (s >> m) & 1:
                p1[:, m] = p1[:, m] + ps
            else:
                p0[:, m] = p0[:, m] + ps
    with np.errstate(all="ignore"):
        return R.synth_log(p0 / p1)


def polarized_ullr(cid, snr_db, seed, trial0, num_sym, with_err=False):
    """(u-LLRs [S][nb], message bits [S][nb]) of symbols trial0 .. trial0+num_sym-1 (+ genie_llr_err's bounds)."""
    nb = R.nbits(cid)
    trials = np.arange(trial0, trial0 + num_sym, dtype=np.uint64)
    u = R.construction_message(seed, trials, nb)
    x = R.polar_encode(u)
    sym = (x.astype(np.int64) << np.arange(nb)).sum(axis=1)
    s = sigma(snr_db)
    y = R.points(cid)[sym] + s * R.symbol_noise(seed, trials, 1)[:, 0]
    if with_err:
        _, ul, err = genie_llr_err(bicm_llr(y, s * s, cid), u)
        return ul, u, err
    _, ul = genie_llr(bicm_llr(y, s * s, cid), u)
    return ul, u


def llr_bins(ul):
    """Constellation.m:331-341: clip to +-100 (NaN -> -100), floor((u + 100) / 0.25) (0-based)."""
    v = np.where(np.isnan(ul), -100.0, np.maximum(ul, -100.0))
    v = np.minimum(v, 100.0)
    return np.floor((v + 100.0) / 0.25).astype(np.int64)


def bin_range(ul, err):
    """(lowest, highest) bin the u-LLR can reach when it moves by up to err (plus 1e-9): clipping and NaN -> bin 0 as
    llr_bins; an infinite or NaN bound reaches every bin."""
    with np.errstate(invalid="ignore"):
        e = err + 1e-9
        lo = llr_bins(np.where(np.isnan(ul), ul, ul - e))
        hi = llr_bins(np.where(np.isnan(ul), ul, ul + e))
    wide = ~np.isfinite(err)
    return np.where(wide, 0, lo), np.where(wide, BINS - 1, hi)


def polarized_counts(cid, snr_db, seed, trial0, num_sym):
    ul, u = polarized_ullr(cid, snr_db, seed, trial0, num_sym)
    nb = ul.shape[1]
    cnt = np.zeros((nb, BINS, 2), np.uint64)
    b = llr_bins(ul)
    for j in range(nb):
        np.add.at(cnt[j], (b[:, j], u[:, j]), 1)
    return cnt


def capacity_from_counts(cnt):
    """Constellation.m:336-366 on counts [nb][801][2] -> [nb]."""
    cnt = np.asarray(cnt, np.float64)
    out = np.zeros(cnt.shape[0])
    for j in range(cnt.shape[0]):
        n0, n1 = cnt[j, :, 0].sum(), cnt[j, :, 1].sum()
        py = (cnt[j, :, 0] + cnt[j, :, 1]) / (n0 + n1)
        with np.errstate(all="ignore"):
            p0, p1 = cnt[j, :, 0] / n0, cnt[j, :, 1] / n1
        hy = hu = 0.0
        for b in range(cnt.shape[1]):
            if py[b] > 0:
                hy = hy + math.log2(py[b]) * py[b] * (-1)
            if p0[b] > 0:
                hu = hu + 0.5 * math.log2(p0[b]) * p0[b] * (-1)
            if p1[b] > 0:
                hu = hu + 0.5 * math.log2(p1[b]) * p1[b] * (-1)
        out[j] = min(hy - hu, 1.0)
    return out


# ---- the driver (main_GA_CC_Comparison.m) ---------------------------------------------------------------------------
def rate_walk(bler, rates, snr_vec, target, nbits):
    """The SNR walk of main_GA_CC_Comparison.m:34-66 over a precomputed bler[snr][rate] table -> (snr_needed, ebno_needed,
    flags). Deviations (flags): 1 = the first SNR tried already meets the target ('Possibly too high starting SNR': the
    reference waits for a key press and interpolates with a stale estimate), 2 = the grid ends before the target is met;
    both give NaN."""
    nr = len(rates)
    snr_needed = np.full(nr, np.nan)
    ebno = np.full(nr, np.nan)
    flags = np.zeros(nr, np.int64)
    start = 0
    for r in range(nr):
        idx, prev = None, None
        for si in range(start, len(snr_vec)):
            if bler[si, r] < target:
                idx = si
                break
            prev = bler[si, r]
        if idx is None:
            flags[r] = 2
            start = max(len(snr_vec) - 2, 0)
            continue
        if idx == start:
            flags[r] = 1
        else:
            b = bler[idx, r]
            snr_needed[r] = (snr_vec[idx] * math.log(prev / target) + snr_vec[idx - 1] * math.log(target / b)) / math.log(prev / b)
            ebno[r] = snr_needed[r] - 10 * math.log10(rates[r]) - 10 * math.log10(nbits)
        start = max(idx - 1, 0)
    return snr_needed, ebno, flags
