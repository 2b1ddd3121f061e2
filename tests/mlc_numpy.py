"""numpy restatement of the multi-level coding (MLC) receiver over set-partition ASK (include/polar_synth.h, PolarM
main_MC_CC_Comparison.m:55-62, 98-110, PolarCode.m:155-161, 180-190, 870-914, Constellation.m:95-121).

The fixed-order exp / log / sin / cos of polar_synth.h are ported operation for operation; Python floats are IEEE doubles
and numpy's element-wise operations are correctly rounded and never contracted, so every double here is the device's bit
for bit. The counter-based generator (Philox4x32-10) is tests/test_bicm.py's `_philox` on arrays; tests/test_mlc.py checks the
two against each other, and the symbol noise against test_bicm's libm evaluation `_oracle_symbol_noise`."""
import numpy as np

BPSK, ASK4_GRAY, ASK8_GRAY, ASK16_GRAY, ASK4_SP, ASK8_SP, ASK16_SP = 4, 1, 2, 3, 5, 6, 7
NAMES = {"bpsk": 4, "ask4-gray": 1, "ask8-gray": 2, "ask16-gray": 3, "ask4-sp": 5, "ask8-sp": 6, "ask16-sp": 7}
_GRAY = {1: ([-3, -1, 3, 1], 5.0), 2: ([-7, -5, -1, -3, 7, 5, 1, 3], 21.0),
         3: ([-15, -13, -9, -11, -1, -3, -7, -5, 15, 13, 9, 11, 1, 3, 7, 5], 85.0)}
_M32 = np.uint64(0xFFFFFFFF)


def nbits(cid):
    return {4: 1, 1: 2, 5: 2, 2: 3, 6: 3, 3: 4, 7: 4}[cid]


def points(cid):
    """polar_const_point(cid, s) / polar_const_norm(cid) for every s (Constellation.m:19-32, 80)."""
    ns = 1 << nbits(cid)
    if cid == BPSK:
        raw = [1.0, -1.0]
    elif cid in _GRAY:
        lv, div = _GRAY[cid]
        raw = [float(v) / np.sqrt(div) for v in lv]
    else:
        div = {4: 5.0, 8: 21.0, 16: 85.0}[ns]
        raw = [float(2 * s - (ns - 1)) / np.sqrt(div) for s in range(ns)]
    acc = 0.0
    for x in raw:
        acc = acc + x * x
    norm = float(np.sqrt(acc / ns))
    return np.array([x / norm for x in raw])


# ---- polar_synth.h, vectorised --------------------------------------------------------------------------------------
def philox(c0, c1, c2, c3, k0, k1):
    c = [np.asarray(v, np.uint64) & _M32 for v in (c0, c1, c2, c3)]
    c = np.broadcast_arrays(*c)
    c = [a.copy() for a in c]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c


def u01(hi, lo):
    k = ((hi << np.uint64(32)) | lo) >> np.uint64(12)
    return (k.astype(np.float64) + 0.5) * 2.220446049250313e-16


def synth_log(x):
    x = np.asarray(x, np.float64)
    u = x.view(np.uint64)
    e = ((u >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 1023
    m = ((u & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    big = m > 1.4142135623730951
    m = np.where(big, m * 0.5, m)
    e = np.where(big, e + 1, e)
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = np.full_like(z, 1.0 / 25.0)
    for d in (23.0, 21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = p * z + 1.0 / d
    p = p * z + 1.0
    return e.astype(np.float64) * 0.6931471805599453 + 2.0 * s * p


def synth_sincos2pi(u):
    t = u * 4.0
    q = t.astype(np.int64)
    f = t - q.astype(np.float64)
    swap = f > 0.5
    f = np.where(swap, 1.0 - f, f)
    x = f * 1.5707963267948966
    z = x * x
    ps = np.full_like(z, 1.0 / 355687428096000.0)
    for d in (1307674368000.0, 6227020800.0, 39916800.0, 362880.0, 5040.0, 120.0, 6.0):
        ps = 1.0 / d - ps * z
    ps = 1.0 - ps * z
    s0 = x * ps
    pc = np.full_like(z, 1.0 / 20922789888000.0)
    for d in (87178291200.0, 479001600.0, 3628800.0, 40320.0, 720.0, 24.0, 2.0):
        pc = 1.0 / d - pc * z
    pc = 1.0 - pc * z
    c0 = pc
    s0, c0 = np.where(swap, c0, s0), np.where(swap, s0, c0)
    so = np.select([q == 0, q == 1, q == 2], [s0, c0, -s0], -c0)
    co = np.select([q == 0, q == 1, q == 2], [c0, -s0, -c0], s0)
    return so, co


def exp_neg(x):
    """polar_synth_exp_neg (x <= 0)."""
    x = np.asarray(x, np.float64)
    t = x * 1.4426950408889634
    k = np.trunc(t - 0.5)
    k = np.where(x < -708.0, 0.0, k).astype(np.int64)
    kd = k.astype(np.float64)
    r = (x - kd * 0.693147180369123816490) - kd * 1.90821492927058770002e-10
    p = np.full_like(r, 1.0 / 6227020800.0)
    for d in (479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0):
        p = p * r + 1.0 / d
    p = p * r + 0.5
    p = p * r + 1.0
    p = p * r + 1.0
    return np.where(x < -708.0, 0.0, p * np.ldexp(1.0, k))


def symbol_noise(seed, trials, nsym):
    """polar_synth_symbol_noise for trials [T] x symbols [nsym]."""
    trials = np.asarray(trials, np.uint64)[:, None]
    sym = np.arange(nsym, dtype=np.uint64)[None, :]
    r = philox(sym >> np.uint64(1), trials & _M32, trials >> np.uint64(32), 2, seed & 0xFFFFFFFF, seed >> 32)
    u1, u2 = u01(r[0], r[1]), u01(r[2], r[3])
    rad = np.sqrt(-2.0 * synth_log(u1))
    sn, cs = synth_sincos2pi(u2)
    return np.where((sym & np.uint64(1)) == 1, rad * sn, rad * cs)


def sweep_info(seed, trials, K):
    """The K info bits of the sweep (polar_synth_info_word keyed by the trial: info_block_div = 1)."""
    trials = np.asarray(trials, np.uint64)[:, None]
    i = np.arange(K, dtype=np.uint64)[None, :]
    r = philox(i >> np.uint64(7), trials & _M32, trials >> np.uint64(32), 1, seed & 0xFFFFFFFF, seed >> 32)
    k = i & np.uint64(127)
    w = np.select([(k >> np.uint64(5)) == j for j in range(4)], r)
    return ((w >> (k & np.uint64(31))) & np.uint64(1)).astype(np.uint8)


def construction_message(seed, trials, N):
    """The N message bits of a construction run (polar_synth_mc_info_word), layer-major."""
    trials = np.asarray(trials, np.uint64)[:, None]
    j = np.arange(N, dtype=np.uint64)[None, :]
    q = j >> np.uint64(5)
    r = philox(q >> np.uint64(2), trials & _M32, trials >> np.uint64(32), 3, seed & 0xFFFFFFFF, seed >> 32)
    w = np.select([(q & np.uint64(3)) == t for t in range(4)], r)
    return ((w >> (j & np.uint64(31))) & np.uint64(1)).astype(np.uint8)


def sigma_n0(snr_db):
    s = np.sqrt(1.0 / 2) * 10.0 ** (-snr_db / 20)          # std::pow vs numpy power: checked equal for the axis values used
    return float(s), float(s * s)


# ---- the receiver ---------------------------------------------------------------------------------------------------
def polar_encode(u):
    """PolarCode.polar_encode (PolarCode.m:855-867) on rows [B][M] of 0/1."""
    u = np.asarray(u, np.uint8)
    if u.shape[-1] == 1:
        return u.copy()
    return np.concatenate([polar_encode(u[..., 0::2] ^ u[..., 1::2]), polar_encode(u[..., 1::2])], axis=-1)


def encode(frozen, order, K, info, cid):
    """main_MC_CC_Comparison.m:55-62: info [B][K] -> (component codewords [nb][B][M], coded bits [B][N] in modulation order)."""
    info = np.atleast_2d(np.asarray(info, np.uint8))
    B, N, nb = info.shape[0], len(frozen), nbits(cid)
    M = N // nb
    u = np.zeros((B, N), np.uint8)
    u[:, np.asarray(order[:K], np.int64)] = info
    comps = [polar_encode(u[:, k * M:(k + 1) * M]) for k in range(nb)]
    coded = np.stack(comps, axis=2).reshape(B, N)           # coded(layer:nb:N) = component layer
    return comps, coded


def modulate(comps, cid):
    sym = sum((1 << k) * comps[k].astype(np.int64) for k in range(len(comps)))
    return points(cid)[sym]


def demap(y, n0, k, u_lower, cid):
    """compute_llr_mlc (Constellation.m:95-121) for layer k (0-based): p1 [B][M], u_lower [k][B][M] doubles."""
    pts = points(cid)
    ns = len(pts)
    p0 = np.zeros_like(y)
    p1 = np.zeros_like(y)
    for s in range(ns):
        valid = np.ones(y.shape, bool)
        for m in range(k):
            valid &= float((s >> m) & 1) == u_lower[m]
        d = y - pts[s]
        ad = np.abs(d)
        ps = exp_neg(-(ad * ad) / 2 / n0)
        if (s >> k) & 1:
            p1 = np.where(valid, p1 + ps, p1)
        else:
            p0 = np.where(valid, p0 + ps, p0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return p1 / (p0 + p1)


def cnop(a, b):
    return a * (1 - b) + b * (1 - a)


def vnop(a, b):
    return a * b / (a * b + (1 - a) * (1 - b))


def polar_decode(y, f):
    """PolarCode.polar_decode (:870-887) on rows [B][M]: (u, x)."""
    M = y.shape[-1]
    if M == 1:
        if f[0] == 0:
            # x = (1 - sign(1 - 2y)) / 2 (:873) with the sign of the MLC kernels, (t > 0) - (t < 0): a NaN leaf decides
            # 0.5 (MATLAB's sign(NaN) is NaN; either way the value matches no label bit in the demapper of the next layer)
            t = 1 - 2 * y
            x = (1 - ((t > 0).astype(np.float64) - (t < 0).astype(np.float64))) / 2
        else:
            x = np.zeros_like(y)
        return x, x
    u1, x1 = polar_decode(cnop(y[:, 0::2], y[:, 1::2]), f[: M // 2])
    u2, x2 = polar_decode(vnop(cnop(x1, y[:, 0::2]), y[:, 1::2]), f[M // 2:])
    x = np.empty_like(y)
    x[:, 0::2] = cnop(x1, x2)
    x[:, 1::2] = x2
    return np.concatenate([u1, u2], axis=1), x


def decode(frozen, order, K, y, n0, cid):
    """Multistage SC decoding (main_MC_CC_Comparison.m:98-110): y [B][M] -> the K info decisions as doubles [B][K]."""
    with np.errstate(invalid="ignore", divide="ignore"):
        y = np.atleast_2d(np.asarray(y, np.float64))
        nb = nbits(cid)
        M = y.shape[1]
        frozen = np.asarray(frozen)
        us, xs = [], []
        for k in range(nb):
            p1 = demap(y, n0, k, xs, cid)
            u, x = polar_decode(p1, frozen[k * M:(k + 1) * M])
            us.append(u)
            xs.append(x)
        return np.concatenate(us, axis=1)[:, np.asarray(order[:K], np.int64)]


def polar_decode_monte(y, bits):
    """PolarCode.polar_decode_monte (:897-914) on rows: (x, ber) with x the re-encoding of the true bits."""
    M = y.shape[-1]
    if M == 1:
        b = bits[:, :1]
        ok = ((y > 0.5) & (b == 1)) | ((y <= 0.5) & (b == 0))
        return b.astype(np.float64), (~ok).astype(np.int64)
    x1, e1 = polar_decode_monte(cnop(y[:, 0::2], y[:, 1::2]), bits[:, : M // 2])
    x2, e2 = polar_decode_monte(vnop(cnop(x1, y[:, 0::2]), y[:, 1::2]), bits[:, M // 2:])
    x = np.empty_like(y)
    x[:, 0::2] = cnop(x1, x2)
    x[:, 1::2] = x2
    return x, np.concatenate([e1, e2], axis=1)


def genie_counts(y, msg, n0, cid):
    """Genie-aided MLC construction (PolarCode.m:180-190): per-position error counts over the rows, layer-major [N]."""
    with np.errstate(invalid="ignore", divide="ignore"):
        nb = nbits(cid)
        M = y.shape[1]
        xs, errs = [], []
        for k in range(nb):
            p1 = demap(y, n0, k, xs, cid)
            x, e = polar_decode_monte(p1, msg[:, k * M:(k + 1) * M])
            xs.append(x)
            errs.append(e.sum(0))
        return np.concatenate(errs)


# ---- the synthetic workload -----------------------------------------------------------------------------------------
def synth(frozen, order, K, cid, seed, trials, snr_db):
    """polar_synth_mlc_dev: (symbols [T][M], info [T][K])."""
    info = sweep_info(seed, trials, K)
    comps, _ = encode(frozen, order, K, info, cid)
    sigma, _ = sigma_n0(snr_db)
    z = symbol_noise(seed, trials, comps[0].shape[1])
    return modulate(comps, cid) + z * sigma, info


def construction(N, cid, snr_db, seed, trials):
    nb = nbits(cid)
    M = N // nb
    msg = construction_message(seed, trials, N)
    comps = [polar_encode(msg[:, k * M:(k + 1) * M]) for k in range(nb)]
    sigma, n0 = sigma_n0(snr_db)
    y = modulate(comps, cid) + symbol_noise(seed, trials, M) * sigma
    return genie_counts(y, msg, n0, cid)


def sweep_counters(frozen, order, K, cid, seed, snr_vec, max_runs):
    """The reference's per-run loop (main_MC_CC_Comparison.m:64-118) over trials 0 .. max_runs-1 with an early stop that
    never triggers (max_err >= max_runs): a trial is simulated at a point iff it failed at every point before it (a trial
    decoded at a lower SNR is counted, not simulated). Returns err, run, differing info bits per point."""
    P = len(snr_vec)
    err, bit = np.zeros(P, np.int64), np.zeros(P, np.int64)
    run = np.full(P, max_runs, np.int64)
    alive = np.arange(max_runs, dtype=np.uint64)
    for i, snr in enumerate(snr_vec):
        if len(alive) == 0:
            break
        y, info = synth(frozen, order, K, cid, seed, alive, snr)
        _, n0 = sigma_n0(snr)
        d = decode(frozen, order, K, y, n0, cid)
        nd = (d != info).sum(1)
        err[i] = int((nd > 0).sum())
        bit[i] = int(nd.sum())
        alive = alive[nd > 0]
    return err, run, bit
