"""numpy restatement of rate matching (include/polar_amd.h polar_rm_pattern ... polar_ga_construction_init): the
built-in patterns, the forced-frozen leaves, the recover rule with sequential fp64 additions, the design from a start vector via
ga_numpy.awgn_polarization, and the workload's noise through a few-line C shim around include/polar_synth.h.

Conventions: z = butterfly(u) in natural order (stages u[a] ^= u[a + inc]), coded[i] = z[bitrev(i)], an LLR > 0 means bit 0."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import ga_numpy as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P32 = [0, 1, 2, 4, 3, 5, 6, 7, 8, 16, 9, 17, 10, 18, 11, 19, 12, 20, 13, 21, 14, 22, 15, 23, 24, 25, 26, 28, 27, 29, 30, 31]
SCHEMES = ("puncture", "shorten", "repeat", "nr")
GA_THREADS = 256


def bitrev(i, n):
    return int(format(i, "0%db" % n)[::-1], 2) if n else 0


def butterfly(u):
    """The encoder's stages on rows [..., N] in natural order."""
    z = np.array(u, np.uint8)
    N = z.shape[-1]
    inc = 1
    while inc < N:
        for a in range(N):
            if not a & inc:
                z[..., a] ^= z[..., a + inc]
        inc <<= 1
    return z


def coded_of(u, n):
    z = butterfly(u)
    return z[..., [bitrev(i, n) for i in range(1 << n)]]


def nr_y(n):
    N = 1 << n
    return np.array([bitrev(P32[32 * j // N] * (N // 32) + j % (N // 32), n) for j in range(N)], np.int64)


def pattern(n, E, scheme, Kp=None):
    """(sel [E], known [N]) of a built-in scheme."""
    N = 1 << n
    known = np.zeros(N, np.uint8)
    if scheme == "puncture":
        assert E < N
        sel = N - E + np.arange(E)
    elif scheme == "shorten":
        assert E < N
        sel = np.arange(E)
        known[E:] = 1
    elif scheme == "repeat":
        assert E >= N
        sel = np.arange(E) % N
    elif scheme == "nr":
        assert n >= 5
        y = nr_y(n)
        if E >= N:
            sel = y[np.arange(E) % N]
        elif 16 * Kp <= 7 * E:
            sel = y[np.arange(E) + N - E]
        else:
            sel = y[:E]
            known[y[E:]] = 1
    else:
        raise ValueError(scheme)
    return sel.astype(np.uint16), known


def punctured(n, sel, known):
    p = np.ones(1 << n, bool)
    p[np.asarray(sel, np.int64)] = False
    return p & (np.asarray(known) == 0)


def forced(n, sel, known):
    """Mask [N] by leaf index: the leaves above a known position, and the zero-capacity leaves of the punctured set."""
    N = 1 << n
    f = np.zeros(N, np.uint8)
    for p in np.nonzero(known)[0]:
        j = bitrev(int(p), n)
        for b in range(N):
            if b & j == j:
                f[b] = 1
    row = punctured(n, sel, known)
    for _ in range(n):
        c1, c2 = row[0::2], row[1::2]
        row = np.concatenate([c1 | c2, c1 & c2])
    for i in range(N):
        if row[bitrev(i, n)]:
            f[i] = 1
    return f


def widen(rx, fmt):
    """The float64 of the same value: f64 / f32 / f16 arrays as they are, bf16 as uint16 patterns."""
    if fmt == "bf16":
        return (np.asarray(rx, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    if fmt == "f16" and np.asarray(rx).dtype == np.uint16:
        return np.asarray(rx).view(np.float16).astype(np.float64)
    return np.asarray(rx).astype(np.float64)


def recover(rx, sel, known, short_llr=1000.0):
    """rx float64 [B, E] -> llr [B, N]: short_llr at a known position, else +0.0 plus the sources in ascending e, one addition
    at a time."""
    rx = np.asarray(rx, np.float64)
    N = len(known)
    out = np.zeros((rx.shape[0], N), np.float64)            # (+0.0)
    with np.errstate(invalid="ignore"):
        for e, p in enumerate(np.asarray(sel, np.int64)):
            out[:, p] = out[:, p] + rx[:, e]
    out[:, np.asarray(known) != 0] = short_llr
    return out


def snr_sqrt_linear_rm(K, E, ebno_db):
    return math.pow(10.0, ebno_db / 20) * math.sqrt(float(K) / float(E))


def prefix_sums(terms):
    """The device's summation of N terms: 256 contiguous chunks, each summed in order on top of the sum of the chunks before it."""
    N = len(terms)
    per = (N + GA_THREADS - 1) // GA_THREADS
    part = []
    for t in range(GA_THREADS):
        s = 0.0
        for r in range(min(N, t * per), min(N, t * per + per)):
            s = s + terms[r]
        part.append(s)
    out = np.zeros(N)
    acc0 = 0.0
    for t in range(GA_THREADS):
        acc = acc0
        for r in range(min(N, t * per), min(N, t * per + per)):
            acc = acc + terms[r]
            out[r] = acc
        acc0 = acc0 + part[t]
    return out


def design(n, K, crc, E, scheme, ebno_db, fwd, inv):
    """The design of PolarCode.from_gauss_approx_rm -> dict(sel, known, forced, channels, order, prefix, frozen, bler)."""
    N, k = 1 << n, K + crc
    sel, known = pattern(n, E, scheme, k)
    f = forced(n, sel, known)
    init = (4 * (K / E) * 10 ** (ebno_db / 10)) * np.bincount(sel, minlength=N).astype(np.float64)
    init[known != 0] = 1e4
    ch = G.awgn_polarization(init, n, fwd, inv)[G.bitrev(n)]
    free = np.nonzero(f == 0)[0]
    order = np.concatenate([free[np.argsort(-ch[free], kind="stable")], np.nonzero(f)[0]])
    prefix = prefix_sums(G.qfunc_terms(ch[order]))
    frozen = np.ones(N, np.uint8)
    frozen[order[:k]] = 0
    return dict(sel=sel, known=known, forced=f, channels=ch, order=order.astype(np.uint16), prefix=prefix, frozen=frozen,
                bler=float(prefix[k - 1]))


# ---- the workload's noise: include/polar_synth.h through a C shim ---------------------------------------------------
SHIM_SRC = r"""
#include "polar_synth.h"
void rm_shim_rx(uint64_t seed, uint64_t trial, int E, double s, const uint8_t *tx, double *rx) {
    for (int e = 0; e < E; ++e) {
        double z[2];
        polar_synth_noise_pair(seed, trial, (uint32_t)(e >> 1), &z[0], &z[1]);
        rx[e] = polar_synth_llr(s, tx[e], z[e & 1]);
    }
}
"""


def build_shim(tmp_dir):
    """Compiles the shim with the host compiler into tmp_dir and returns rx(seed, trials, s, tx [B, E]) -> float64 [B, E]."""
    src, so = os.path.join(str(tmp_dir), "rm_shim.c"), os.path.join(str(tmp_dir), "rm_shim.so")
    open(src, "w").write(SHIM_SRC)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           src, "-o", so, "-lm"])
    lib = C.CDLL(so)

    def rx(seed, trials, s, tx):
        tx = np.ascontiguousarray(tx, np.uint8)
        out = np.zeros(tx.shape, np.float64)
        for r, t in enumerate(trials):
            lib.rm_shim_rx(C.c_uint64(seed), C.c_uint64(int(t)), C.c_int(tx.shape[1]), C.c_double(s),
                           tx[r].ctypes.data_as(C.POINTER(C.c_uint8)), out[r].ctypes.data_as(C.POINTER(C.c_double)))
        return out
    return rx
