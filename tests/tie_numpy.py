"""The list walk of decode_scl_llr with the reference's own tie rule, in three arithmetics — the model behind the tests of rows
whose fork metrics tie (tests/test_tie_model.py, tests/test_gpu_ties.py).

A plain restatement of PolarCode.cpp:130-190, 259-295, 415-607, 609-644: path indices come from the LIFO stack of inactive
indices (the stack is filled 0 .. L-1, so the first path is L-1; a killed path's index is pushed back, a clone takes the top),
the 2 L fork metrics are laid out by path index (forks 2 l and 2 l + 1), the threshold is the rho-th best of them, the forks
better than the threshold continue, then those equal to it in fork-index order until rho continue (:528-553), and the word
returned is the first path in index order with the smallest metric among those that pass the CRC (:609-644; path 0 where no
metric is below DBL_MAX). It is not the copy-on-write machinery — every path owns its arrays — and it is not scl_list_numpy,
which raises TieError wherever the tie rule would matter.

The walk is always DRIVEN by the fp64 arithmetic (math.exp / math.log, the platform's libm, which is the oracle's: asserted by
the tests on every row they use), so it follows the reference fork by fork. Beside it, it can carry a second arithmetic along
the same paths, and reports at every fork whether the second arithmetic would have kept another set under the same index rule:

  "exact"  rows whose node values are all 0 or at least 40 in magnitude (others raise NotExact). There every reference operation
           is exact: f is min-sum, or log(2 / 2) = 0 for a pair of zeros; g is an integer sum; a leaf adds 0 for the good fork,
           |l| for the bad one (+inf from 709.78 on), log 2 for both forks of a zero leaf. A metric is a + k log 2 with an
           integer-valued a and an integer k, kept as the pair (a, k); two metrics are equal only when the pairs are (+inf
           equals +inf), and otherwise compared by (a1 - a2) + (k1 - k2) log 2 in 50-digit arithmetic.
  "mp"     mpmath at 60 digits, for any row; two fork metrics count as equal when they agree to 1e-40.

A row is EXACTLY DECIDED at list size L when no fork of the walk keeps another set under "exact" than under fp64: the
reference's output then follows from the index rule alone. A row is NOISE-DECIDED when some fork keeps another set under "mp"
than under fp64: the reference's output then rests on the rounding of its own sums.
"""
import functools
import math
import os

import numpy as np

LOG2 = math.log(2.0)


class NotExact(ValueError):
    """The row has a node value strictly between 0 and 40 in magnitude: the "exact" arithmetic does not cover it."""


# ---- fp64: the reference's operations, scalar, through libm ------------------------------------------------------------------
def f64(a, b):
    if 40 > max(abs(a), abs(b)):
        return math.log((math.exp(a + b) + 1) / (math.exp(a) + math.exp(b)))
    sa = -1 if a < 0 else (1 if a > 0 else 0)
    sb = -1 if b < 0 else (1 if b > 0 else 0)
    return float(sa * sb) * min(abs(a), abs(b))


def cost64(x):
    """log(1 + exp(x)); exp overflows to +inf above 709.78"""
    try:
        return math.log(1 + math.exp(x))
    except OverflowError:
        return math.inf


def _f_level(a, b):
    """f over arrays: min-sum where the reference takes it, the scalar libm expression elsewhere"""
    fa, fb = np.abs(a), np.abs(b)
    out = np.sign(a) * np.sign(b) * np.minimum(fa, fb)
    for i in zip(*np.nonzero(np.maximum(fa, fb) < 40)):
        out[i] = f64(float(a[i]), float(b[i]))
    return out


# ---- the second arithmetics ---------------------------------------------------------------------------------------------------
class _Exact:
    name = "exact"

    def __init__(self):
        import mpmath
        self.mp = mpmath.mp.clone()
        self.mp.dps = 50
        self.log2 = self.mp.log(2)
        self.zero = (0.0, 0)

    def nodes(self, llr):
        return None                                        # node values are the fp64 ones: every operation on them is exact

    def check(self, v):
        a = np.abs(v)
        if ((a != 0) & (a < 40)).any():
            raise NotExact("node value %r" % float(a[(a != 0) & (a < 40)][0]))

    def cost(self, x, _node):
        """the leaf term for the fork whose cost is log(1 + exp(x)), x the fp64 leaf value or its negative"""
        if x == 0:
            return (0.0, 1)
        if x > 709.78:
            return (math.inf, 0)
        return (x, 0) if x > 0 else (0.0, 0)

    def add(self, m, c):
        return (m[0] + c[0], m[1] + c[1])

    def cmp(self, p, q):
        """-1: p is the smaller metric, 0: equal, 1: larger"""
        if p == q or (p[0] == math.inf and q[0] == math.inf):
            return 0
        if p[0] == math.inf or q[0] == math.inf:
            return 1 if p[0] == math.inf else -1
        d = (p[0] - q[0]) + (p[1] - q[1]) * LOG2          # (the difference of the a's is exact; decisive unless tiny)
        if abs(d) < 1e-6:
            d = self.mp.mpf(p[0]) - self.mp.mpf(q[0]) + (p[1] - q[1]) * self.log2
        assert d != 0
        return -1 if d < 0 else 1


class _Mp:
    name = "mp"

    def __init__(self):
        import mpmath
        self.mp = mpmath.mp.clone()
        self.mp.dps = 60
        self.tol = self.mp.mpf("1e-40")
        self.zero = self.mp.mpf(0)
        self.inf = self.mp.inf
        self._f = {}

    def nodes(self, llr):
        return [self.mp.mpf(float(x)) for x in llr]

    def f(self, a, b):
        r = self._f.get((a, b))
        if r is None:
            mp = self.mp
            if 40 > max(abs(a), abs(b)):
                r = mp.log((mp.exp(a + b) + 1) / (mp.exp(a) + mp.exp(b)))
            else:
                r = mp.sign(a) * mp.sign(b) * min(abs(a), abs(b))
            self._f[(a, b)] = r
        return r

    def cost(self, _x, node):
        """node: the mp value whose log(1 + exp(.)) is the term"""
        if node > 709.78:
            return self.inf
        return self.mp.log(1 + self.mp.exp(node))

    def add(self, m, c):
        return m + c

    def cmp(self, p, q):
        if p == q:
            return 0
        if p == self.inf or q == self.inf:
            return 1 if p == self.inf else -1
        d = p - q
        if abs(d) <= self.tol * max(1, abs(p), abs(q)):
            return 0
        return -1 if d < 0 else 1


def _cmp64(p, q):
    return 0 if p == q else (-1 if p < q else 1)


def keep_set(forks, rho, cmp):
    """PolarCode.cpp:521-553 on fork metrics (smaller = better; None = an inactive path's fork): the fork indices that continue.
    The forks better than the rho-th best all continue; those equal to it continue in index order until rho do."""
    live = [i for i, m in enumerate(forks) if m is not None]
    ranked = sorted((forks[i] for i in live), key=functools.cmp_to_key(cmp))
    thr = ranked[rho - 1]
    kept = [i for i in live if cmp(forks[i], thr) < 0]
    assert len(kept) < rho
    for i in live:
        if len(kept) == rho:
            break
        if cmp(forks[i], thr) == 0:
            kept.append(i)
    return frozenset(kept)


class Fork:
    """One unfrozen leaf of the walk: phi, the number of forks kept (rho) and offered, the fp64 margin between the last kept and
    the first dropped metric (None where every fork continues; 0.0 at a tie; inf - inf counts as a tie) with the kept metric it
    is relative to, and whether the second arithmetic keeps another set."""
    __slots__ = ("phi", "rho", "offered", "margin", "at", "differs")

    def margin_ulps(self):
        if self.margin is None or self.margin == 0 or not math.isfinite(self.at) or not math.isfinite(self.margin):
            return self.margin
        return self.margin / math.ulp(self.at if self.at != 0 else 1.0)


class Result:
    """info [K] the decoded word; paths: the list at the end in path-index order, dicts (index, u [N], info [K], pm fp64, crc_ok);
    winner: the path index returned; forks: one Fork per unfrozen leaf."""

    def __init__(self, info, paths, winner, forks):
        self.info, self.paths, self.winner, self.forks = info, paths, winner, forks

    def exactly_decided(self):
        return not any(f.differs for f in self.forks)

    def first_difference(self):
        for f in self.forks:
            if f.differs:
                return f
        return None

    def tie_forks(self):
        """forks whose cut lies on an fp64 tie"""
        return [f for f in self.forks if f.margin is not None and (f.margin == 0 or math.isnan(f.margin))]

    def sorted_list(self):
        """the paths in the row order of decode_scl_llr_list: CRC pass first, then the smaller metric, then the path index"""
        return sorted(self.paths, key=lambda p: (not p["crc_ok"], p["pm"], p["index"]))


def walk(code, llr, L, second=None):
    """code: scl_list_numpy.Code; llr [N]; second: None, "exact" or "mp" -> Result. Arrays are indexed by path index."""
    import scl_list_numpy as sl
    n, N = code.n, code.N
    ar = {None: None, "exact": _Exact, "mp": _Mp}[second]
    ar = ar() if ar else None
    llr = np.asarray(llr, np.float64)
    A = [np.zeros((L, N >> lam)) for lam in range(n + 1)]
    CL = [np.zeros((L, N >> lam), np.uint8) for lam in range(n + 1)]
    CR = [np.zeros((L, N >> lam), np.uint8) for lam in range(n + 1)]
    U = np.zeros((L, N), np.uint8)
    pm, pm2 = [0.0] * L, [ar.zero if ar else None] * L
    A2 = None                                               # "mp": per path, per level, a list of mp values
    stack = list(range(L))                                  # _inactivePathIndices: top = the end of the list
    l0 = stack.pop()
    active = [l0]
    A[0][l0] = llr
    if second == "exact":
        ar.check(llr)
    if second == "mp":
        A2 = {l0: [ar.nodes(llr)] + [[ar.zero] * (N >> lam) for lam in range(1, n + 1)]}
    forks = []
    for phi in range(N):
        lam_top = 1 if phi == 0 else n - ((phi & -phi).bit_length() - 1)
        for lam in range(lam_top, n + 1):
            a, b = A[lam - 1][active, 0::2], A[lam - 1][active, 1::2]
            isg = (phi >> (n - lam)) & 1
            A[lam][active] = (1 - 2 * CL[lam][active].astype(np.float64)) * a + b if isg else _f_level(a, b)
            if second == "exact":
                ar.check(A[lam][active])
            if A2 is not None:
                for l in active:
                    a2, b2 = A2[l][lam - 1][0::2], A2[l][lam - 1][1::2]
                    if isg:
                        A2[l][lam] = [(y - x if c else x + y) for x, y, c in zip(a2, b2, CL[lam][l])]
                    else:
                        A2[l][lam] = [ar.f(x, y) for x, y in zip(a2, b2)]
        if code.frozen[phi]:
            for l in active:
                v = float(A[n][l, 0])
                pm[l] += cost64(-v)
                if ar is not None:
                    pm2[l] = ar.add(pm2[l], ar.cost(-v, -A2[l][n][0] if A2 else None))
            _set_bits(CL, CR, U, n, phi, active, np.zeros(len(active), np.uint8))
            continue
        # continuePaths_UnfrozenBit
        m64, m2 = [None] * (2 * L), [None] * (2 * L)
        for l in active:
            v = float(A[n][l, 0])
            m64[2 * l], m64[2 * l + 1] = pm[l] + cost64(-v), pm[l] + cost64(v)
            if ar is not None:
                v2 = A2[l][n][0] if A2 else None
                m2[2 * l] = ar.add(pm2[l], ar.cost(-v, -v2 if A2 else None))
                m2[2 * l + 1] = ar.add(pm2[l], ar.cost(v, v2))
        rho = min(L, 2 * len(active))
        kept = keep_set(m64, rho, _cmp64)
        fk = Fork()
        fk.phi, fk.rho, fk.offered = phi, rho, 2 * len(active)
        fk.margin = fk.at = None
        if 2 * len(active) > rho:
            ranked = sorted(m for m in m64 if m is not None)
            fk.at = ranked[rho - 1]
            fk.margin = 0.0 if ranked[rho] == ranked[rho - 1] else ranked[rho] - ranked[rho - 1]
        fk.differs = bool(ar is not None and keep_set(m2, rho, ar.cmp) != kept)
        forks.append(fk)
        for l in active:                                    # kills first, in index order (:555-560)
            if 2 * l not in kept and 2 * l + 1 not in kept:
                stack.append(l)
                pm[l] = 0.0
        now, bits = [], []
        for l in range(L):                                  # (:562-605)
            k0, k1 = 2 * l in kept, 2 * l + 1 in kept
            if not (k0 or k1):
                continue
            if k0 and k1:
                lp = stack.pop()
                for X in A + CL + CR + [U]:
                    X[lp] = X[l]
                if A2 is not None:
                    A2[lp] = [list(x) for x in A2[l]]
                pm[l], pm2[l] = m64[2 * l], m2[2 * l]
                pm[lp], pm2[lp] = m64[2 * l + 1], m2[2 * l + 1]
                now += [l, lp]
                bits += [0, 1]
            else:
                b = 0 if k0 else 1
                pm[l], pm2[l] = m64[2 * l + b], m2[2 * l + b]
                now.append(l)
                bits.append(b)
        order = np.argsort(now)
        active = [now[i] for i in order]
        _set_bits(CL, CR, U, n, phi, active, np.asarray(bits, np.uint8)[order])
    out = []
    for l in active:
        info, check = sl.split(code, U[l])
        out.append(dict(index=l, u=U[l].copy(), info=info.copy(), pm=pm[l], crc_ok=bool(sl.crc_ok(code, info, check))))
    winner = _most_probable(out, bool(code.crc))
    by_index = {q["index"]: q for q in out}
    info = by_index[winner]["info"] if winner in by_index else np.zeros(code.K, np.uint8)
    return Result(info, out, winner, forks)


def _most_probable(paths, check_crc):
    """findMostProbablePath (:609-644)"""
    best, best_pm, passed = 0, 1.7976931348623157e308, False
    for q in paths:
        if check_crc and not q["crc_ok"]:
            continue
        passed = True
        if q["pm"] < best_pm:
            best, best_pm = q["index"], q["pm"]
    return best if passed else _most_probable(paths, False)


def _set_bits(CL, CR, U, n, phi, active, bits):
    """the decisions at leaf phi of the paths `active` and, at an odd leaf, recursivelyUpdateC (:457-473)"""
    U[active, phi] = bits
    if not phi & 1:
        CL[n][active, 0] = bits
        return
    CR[n][active, 0] = bits
    lam, ph = n, phi
    while True:
        psi = ph >> 1
        dst = CR[lam - 1] if psi & 1 else CL[lam - 1]
        dst[active, 0::2] = CL[lam][active] ^ CR[lam][active]
        dst[active, 1::2] = CR[lam][active]
        if (psi & 1) and lam - 1 >= 1:
            lam, ph = lam - 1, psi
        else:
            break


# ---- the rows the CPU and the GPU tests share ---------------------------------------------------------------------------------
TIE_C = 45.0                                                # exact in binary16 and bfloat16; 5 above the |x| = 40 window
TIE_SEED = 777
TIE_CODES = {(8, 128, 8): (24, (1, 2, 3, 4, 8, 16, 24, 32)),       # code: (rows, list sizes the GPU tests use)
             (9, 128, 8): (24, (1, 2, 3, 4, 8, 16, 24, 32)),
             (10, 512, 8): (8, (8, 32)),
             (10, 256, 8): (8, (8, 32))}                            # (takes the two-phase head of the fixed-N list-of-32 kernel)
TIE_SNRS = (0.0, 4.0)


def tie_rows(o, code):
    """sign(synthetic noisy codeword) * TIE_C: the rows of a hard-decision front end. o: an oracle_lib.Oracle of `code`."""
    B = TIE_CODES[code][0]
    parts, at = [], 0
    for i, s in enumerate(TIE_SNRS):
        nb = (B - at) if i == len(TIE_SNRS) - 1 else B // len(TIE_SNRS)
        parts.append(o.synth_llr(TIE_SEED, at, nb, o.snr_sqrt_linear(s))[0])
        at += nb
    return np.where(np.concatenate(parts) < 0, -TIE_C, TIE_C)


def pm1_pm3_rows(o):
    """the 20 rows of test_gpu_r1_block.test_exact_zero_leaf_llrs on an oracle of (8, 128, 8)"""
    sg = np.where(o.synth_llr(777, 0, 20, o.snr_sqrt_linear(0.0))[0] < 0, -1.0, 1.0)
    return np.concatenate([sg[:10], 3.0 * sg[10:]])


GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tie_rows.npz")


def golden_key(code, L):
    return "%d_%d_%d_L%d" % (code + (L,))


def load_golden():
    """{(code, L): (indices of the exactly decided rows, the oracle's bits [rows, K])} of tests/golden/tie_rows.npz"""
    z = np.load(GOLDEN_FILE)
    return {(code, L): (z["exact_" + golden_key(code, L)], np.unpackbits(z["bits_" + golden_key(code, L)], axis=1)[:, :code[1]])
            for code, (_, Ls) in TIE_CODES.items() for L in Ls}


_cache = {}


def case(code):
    """(oracle, scl_list_numpy.Code, rows) of one of TIE_CODES, once per process"""
    if code not in _cache:
        import scl_list_numpy as sl
        from oracle_lib import Oracle
        o = Oracle(code[0], code[1], 0.32, code[2], srand=1)
        _cache[code] = (o, sl.Code(o), tie_rows(o, code))
    return _cache[code]


def walked(code, L, r, second="exact"):
    """walk() of row r of a code's tie rows, once per process"""
    k = (code, L, r, second)
    if k not in _cache:
        _, c, x = case(code)
        _cache[k] = walk(c, x[r], L, second)
    return _cache[k]
