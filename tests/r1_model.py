"""A CPU model of the rate-1 quad continuation of the list-of-32 kernels (polar_amd/csrc/polar_scl_leaf.inc): which
leaves the host marks, and how many continuations a wave must finish in one step ("committed") and give up ("discarded").

The decode is the plain numpy list decoder of tests/scl_list_numpy.py (same loop, same arithmetic, TieError where the result would
depend on the reference's tie rule), which here also records, per unfrozen leaf of a codeword, what the kernel's tests see:
  fast   the exact fast-path condition of a leaf step: list full, and the largest good-fork metric PM + log(1 + e^-|llr|) below the
         smallest lower bound (PM + |llr|)(1 - 2^-40) of a bad-fork metric;
  hi     the sufficient test the continuation runs on positions 1 .. 3: the same two numbers compared by their HIGH WORDS only
         (colliding high words give the block up; the loop's exact reductions decide those);
  zero   some path's leaf LLR is exactly 0 (stored magnitude 1.0: it decides 0 whatever its sign bit, the block is given up).
A wave holds two consecutive codewords (2 w, 2 w + 1; the last one alone when B is odd) and every test must hold in both.
numpy's exp / log are not the device's to the last bit (about 1e-13 relative in the metrics): a count can differ only where a
metric lies that close to the other side of a comparison, which the seeded inputs of the tests do not do."""
import numpy as np

from scl_list_numpy import TieError, f_node, g_node, leaf_cost

C40 = 0.99999999999909050530          # 1 - 2^-40, as the kernel


def marks(frozen, weak=None):
    """rb per leaf (0, 2 or 3), the host's rule (derive_tables): the largest aligned block of unfrozen leaves starting there with
    no weak leaf and no leaf other than its last at (t & 31) == 31; a failing octet is shrunk to its quads; leaf 4 of a marked
    octet carries 2."""
    frozen = np.asarray(frozen, np.uint8)
    N = len(frozen)
    rb = np.zeros(N, np.int64)
    if N < 16:
        return rb
    weak = np.zeros(N, bool) if weak is None else np.asarray(weak, bool)
    t = np.concatenate([[0], np.cumsum(frozen == 0)])

    def ok(i0, Z):
        if i0 + Z > N:
            return False
        for i in range(i0, i0 + Z):
            if frozen[i] or weak[i] or (i < i0 + Z - 1 and (t[i] & 31) == 31):
                return False
        return True

    i = 0
    while i < N:
        if i % 8 == 0 and ok(i, 8):
            rb[i], rb[i + 4] = 3, 2
            i += 8
            continue
        if ok(i, 4):
            rb[i] = 2
        i += 4
    return rb


def weak_leaves(frozen):
    """The host's classification: an unfrozen leaf whose capacity over a BEC(1/2) is below 1e-3."""
    frozen = np.asarray(frozen, np.uint8)
    n = int(np.log2(len(frozen)))
    z, om = np.array([0.5]), np.array([0.5])
    for _ in range(n):
        z2, om2 = np.empty(2 * len(z)), np.empty(2 * len(z))
        z2[0::2], om2[0::2] = 2 * z - z * z, om * om
        z2[1::2], om2[1::2] = z * z, om * (1.0 + z)
        z, om = z2, om2
    return (frozen == 0) & (om < 1e-3)


def _hi(x):
    return np.asarray(x, np.float64).view(np.uint64) >> np.uint64(32)


def leaf_tests(frozen, llr, L):
    """One codeword -> (fast, hi, zero), bool arrays over the leaves (False at frozen ones)."""
    frozen = np.asarray(frozen, np.uint8)
    N = len(frozen)
    n = int(np.log2(N))
    A = [np.asarray(llr, np.float64).reshape(1, N)] + [np.zeros((1, N >> lam)) for lam in range(1, n + 1)]
    CL = [np.zeros((1, N >> lam), np.uint8) for lam in range(n + 1)]
    CR = [np.zeros((1, N >> lam), np.uint8) for lam in range(n + 1)]
    pm = np.zeros(1)
    fast, hi, zero = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, bool)
    for phi in range(N):
        lam_top = 1 if phi == 0 else n - ((phi & -phi).bit_length() - 1)
        for lam in range(lam_top, n + 1):
            a, b = A[lam - 1][:, 0::2], A[lam - 1][:, 1::2]
            A[lam] = g_node(a, b, CL[lam]) if (phi >> (n - lam)) & 1 else f_node(a, b)
        v = A[n][:, 0]
        if frozen[phi]:
            pm = pm + leaf_cost(-v)
            bit = np.zeros(len(pm), np.uint8)
        else:
            na = len(pm)
            gmax = np.max(pm + leaf_cost(-np.abs(v)))
            bmin = np.min((pm + np.abs(v)) * C40)
            fast[phi] = na == L and gmax < bmin
            hi[phi] = na == L and _hi(gmax) < _hi(bmin)
            zero[phi] = bool((v == 0).any())
            m = np.concatenate([pm + leaf_cost(-v), pm + leaf_cost(v)])
            keep = np.argsort(m, kind="stable")
            if 2 * na > L:
                if m[keep[L - 1]] == m[keep[L]]:
                    raise TieError("fork metrics %d and %d are equal at leaf %d" % (L, L + 1, phi))
                keep = np.sort(keep[:L])
            src, bit = keep % na, (keep // na).astype(np.uint8)
            A = [x[src] if x.shape[0] == na else x for x in A]
            CL, CR, pm = [x[src] for x in CL], [x[src] for x in CR], m[keep]
        if phi & 1:
            CR[n][:, 0] = bit
            lam, ph = n, phi
            while True:
                psi = ph >> 1
                dst = np.empty((len(pm), 2 * CL[lam].shape[1]), np.uint8)
                dst[:, 0::2] = CL[lam] ^ CR[lam]
                dst[:, 1::2] = CR[lam]
                if psi & 1:
                    CR[lam - 1] = dst
                else:
                    CL[lam - 1] = dst
                if (psi & 1) and lam - 1 >= 1:
                    lam, ph = lam - 1, psi
                else:
                    break
        else:
            CL[n][:, 0] = bit
    return fast, hi, zero


def counts(frozen, llr_rows, L, rb=None):
    """(committed, discarded) of one launch over the rows [B, N]: summed over its waves of two consecutive codewords."""
    frozen = np.asarray(frozen, np.uint8)
    N = len(frozen)
    rb = marks(frozen, weak_leaves(frozen)) if rb is None else rb
    tests = [leaf_tests(frozen, r, L) for r in np.asarray(llr_rows, np.float64)]
    committed = discarded = 0
    for w in range(0, len(tests), 2):
        cws = tests[w:w + 2]
        phi = 0
        while phi < N:
            if rb[phi] and all(f[phi] for f, _, _ in cws):
                if all(h[phi + 1:phi + 4].all() and not z[phi:phi + 4].any() for _, h, z in cws):
                    committed += 1
                    phi += 4
                    continue
                discarded += 1
            phi += 1
    return committed, discarded
