"""Frozen sets that no Bhattacharyya / BEC construction produces, and the rows the decoders are compared on over them (DESIGN.md §2
"Non-monotone masks"). Shared by tests/test_mask_cases.py (CPU: coverage and the conditions on the rows) and tests/test_gpu_masks.py.

A constructed mask is an up-set of the bitwise partial order on leaf indices (i below j where the set bits of i are among those of j:
j is then no less reliable). Within an aligned octet that leaves 20 of the 256 frozen patterns (18 of the 254 mixed ones), within a
quad 6 of 16, and the pair (left leaf unfrozen, right leaf frozen) never occurs. Every mask here starts from a constructed rate-1/2
code and only FREEZES leaves of it, so no weak unfrozen leaf appears (r1_model.weak_leaves) and the fast kernels keep the code.

Octet-pattern codes: of the aligned all-unfrozen octets of the base the weaker FRACTION (weaker_octets: ranked by the Bhattacharyya
parameter of the octet's last leaf — index order alone misplaces octets such as 504 .. 511 of N = 1024) is each overwritten with one
mixed pattern of a seeded permutation of 1 .. 254 (bit j set = leaf 8 o + j frozen); as many codes as it takes for every pattern to
appear. Only the weaker part, because a frozen leaf in a very strong channel carries a large |LLR|: the list-size-1 kernels hand a
row to the fallback pass when the root values of an all-frozen node sum above 690, and with every octet overwritten most rows at
3 dB do (their fast kernels would then go untested).

Rows: 48 trials of the oracle's channel at each of two Eb/N0 points. The guard model (tests/guard_numpy.py) drops, on the CPU, every
row that a fast kernel would or nearly would flag: the criteria on the input, any f-node of the SC pass within WINDOW of |x| = 40, and
for the list-size-1 kernels the product criterion with a factor of 10 to spare and the all-frozen sum with 10 to spare.
"""
import numpy as np

import guard_numpy as G
import scl_list_numpy as S

EPS = 0.32
FRACTION = 0.5                   # of the all-unfrozen octets, the weaker ones
PERM_SEED = 254
EBNO = (1.5, 3.0)
B_POINT = 48
SEED0 = 9100                     # code i of a set draws its rows from seed SEED0 + 16 * n + i
PROD_MIN = 1e-8 * 10             # the kernels flag a product below 1e-8
FSUM_MAX = 690.0 - 10            # ... and an all-frozen sum above 690: the sum stands for the product e^-sum, so 10 off the sum is a
                                 # factor e^10 on what the kernels compare (their sums and numpy's differ by parts in 1e13)
WINDOW = 1e-3                    # distance from |x| = 40 at any f-node of the pass (the kernels' window is 4e-9 wide)
CRC = 8
# measure_scan_tol(draws=(0, 1, 2, 3), codes=scan_codes()): the largest deviation of a finite info_llr / ext entry between the exact SCAN
# model and the model with every exp / log result moved by a random relative 1e-13 plus absolute 1e-15, over the exact-mode rows of
# every code at 4 iterations: 5.5e-9 .. 1.02e-8 over the four draws (rows selected at a margin of 1e-5; at 3e-7: 5.6e-9 .. 1.0e-8).
# Ten times the largest, rounded up to one digit. tests/test_mask_cases.py measures a part of it again.
SCAN_TOL = 2e-7
SCAN_MARGIN = 100 * SCAN_TOL
SCAN_ROWS = 32
FLIP_ROWS = 32
FLIP_T = (0, 4)
LIST_N128_ROWS = 48
# what the parametrised tests are collected from without building anything (tests/test_mask_cases.py holds them against the masks)
N_CODES = {11: 7, 10: 13}
EDGE_NAMES = ("a-last-leaf", "a-last-quad", "b-right-half-16", "b-right-half-64", "c-leaf-1", "c-leaf-2", "c-leaf-5", "c-leaf-7",
              "d-n7-weaker", "d-n7-all-but-last", "d-n7-half-tail")
N_SOFT = N_CODES[10] + 6
ADAPTIVE = (1, 4, 32)


class Tables:
    """An explicit code: what scl_list_numpy.Code, PolarCode.from_tables and the oracle's set_tables take. `order` is the unfrozen
    leaves in index order, then the frozen ones; with a CRC the last `crc` unfrozen entries are the check positions and the CRC
    matrix is the oracle's for (K, crc)."""

    def __init__(self, name, n, frozen, crc=0, seed=0):
        self.name, self.n, self.N, self.crc, self.seed = name, n, 1 << n, crc, seed
        self._frozen = np.asarray(frozen, np.uint8).copy()
        self._frozen.setflags(write=False)
        unf = np.flatnonzero(self._frozen == 0)
        self.K = len(unf) - crc
        self._order = np.concatenate([unf, np.flatnonzero(self._frozen)]).astype(np.uint16)
        self._o = None

    def __repr__(self):
        return self.name

    def frozen(self):
        return self._frozen

    def order(self):
        return self._order

    def oracle(self):
        if self._o is None:
            from oracle_lib import Oracle
            self._o = Oracle(self.n, self.K, EPS, self.crc, srand=1)
            self._o.set_tables(self._frozen, self._order)
        return self._o

    def crc_matrix(self):
        return self.oracle().crc_matrix()

    def with_crc(self, crc=CRC):
        return Tables(self.name + "+crc%d" % crc, self.n, self._frozen, crc, self.seed)

    def handle(self):
        """The device handle (PolarCode.from_tables); a weak-leaf warning is an error here."""
        import warnings
        import polar_amd
        with warnings.catch_warnings():
            warnings.simplefilter("error", polar_amd.PolarWeakLeavesWarning)
            return polar_amd.PolarCode.from_tables(self.n, self.K, self.crc, self._frozen, self._order,
                                                   self.crc_matrix() if self.crc else None)


_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def base_frozen(n):
    def make():
        from oracle_lib import Oracle
        f = Oracle(n, 1 << (n - 1), EPS, 0, srand=1).frozen()
        f.setflags(write=False)
        return f
    return _once(("base", n), make)


def free_blocks(frozen, size):
    """The aligned blocks of `size` leaves with no frozen leaf, in index order."""
    return np.flatnonzero(~np.asarray(frozen, bool).reshape(-1, size).any(axis=1))


def put_octet(frozen, o, pattern):
    frozen[8 * o:8 * o + 8] = (pattern >> np.arange(8)) & 1


def bec_z(n, eps=EPS):
    """The Bhattacharyya parameters of the 2^n leaves over a BEC(eps), in decoding order."""
    z = np.array([eps])
    for _ in range(n):
        z2 = np.empty(2 * len(z))
        z2[0::2], z2[1::2] = 2 * z - z * z, z * z
        z = z2
    return z


def weaker_octets(base):
    """The weaker FRACTION of the all-unfrozen octets of a base mask, in index order. An octet is as strong as its last leaf (the one
    whose LLR is largest when frozen); index order alone is no measure of it (leaf 511 of N = 1024 has nine 1-bits)."""
    free = free_blocks(base, 8)
    z = bec_z(int(np.log2(len(base))))[8 * free + 7]
    return np.sort(free[np.argsort(-z, kind="stable")[:int(len(free) * FRACTION)]])


def patterns():
    return np.random.default_rng(PERM_SEED).permutation(np.arange(1, 255))


def octet_codes(n):
    """The octet-pattern codes of block length 2^n."""
    def make():
        base = base_frozen(n)
        kept = weaker_octets(base)
        perm, m = patterns(), len(kept)
        out = []
        for c in range(-(-254 // m)):
            f = base.copy()
            for k, o in enumerate(kept):
                put_octet(f, o, int(perm[(c * m + k) % 254]))
            out.append(Tables("octets-n%d-%d" % (n, c), n, f, seed=SEED0 + 16 * n + c))
        return out
    return _once(("octets", n), make)


def _edge(name, n, edit, seed):
    f = base_frozen(n).copy()
    edit(f)
    return Tables(name, n, f, seed=SEED0 + 1000 + seed)


def straddling_octet(frozen):
    """The first all-unfrozen octet in which an unfrozen leaf other than the last is the 32nd decision of a history word, whichever
    single leaf of it is frozen: t0 leaves are unfrozen before it, its leaves count t0 .. t0 + 6, and (t & 31) == 31 for one of the
    first five."""
    t = np.concatenate([[0], np.cumsum(np.asarray(frozen) == 0)])
    for o in free_blocks(frozen, 8):
        if 27 <= (t[8 * o] & 31) <= 30:
            return int(o)
    raise ValueError("no all-unfrozen octet straddles a history word")


def edge_masks():
    """The hand-stated masks: {name: Tables}. N = 1024 but for the three N = 128 masks of the whole-list comparison."""
    def make():
        n, N = 10, 1024
        base = base_frozen(n)
        out = []

        def last_leaf(f):
            f[N - 1] = 1

        def last_quad(f):
            f[N - 4:] = 1
        out += [_edge("a-last-leaf", n, last_leaf, 0), _edge("a-last-quad", n, last_quad, 1)]
        for k, half in enumerate((16, 64)):
            # the first all-unfrozen block of that size that is a right child; its left sibling keeps its unfrozen leaves
            b = int([v for v in free_blocks(base, half) if v & 1 and not base[(v - 1) * half:v * half].all()][0])

            def right_half(f, b=b, half=half):
                f[b * half:(b + 1) * half] = 1
            out.append(_edge("b-right-half-%d" % half, n, right_half, 2 + k))
        o = straddling_octet(base)
        for k, pos in enumerate((1, 2, 5, 7)):
            out.append(_edge("c-leaf-%d" % pos, n, lambda f, pos=pos: put_octet(f, o, 1 << pos), 4 + k))
        n7 = base_frozen(7)
        free7, perm = free_blocks(n7, 8), patterns()

        def weaker(f):
            for k, oc in enumerate(free7[:max(2, len(free7) // 2)]):
                put_octet(f, oc, int(perm[k]))

        def all_but_last(f):
            for k, oc in enumerate(free7[:-1]):
                put_octet(f, oc, int(perm[100 + k]))

        def half_and_tail(f):
            b = int([v for v in free_blocks(n7, 16) if v & 1 and not n7[(v - 1) * 16:v * 16].all()][0])
            f[16 * b:16 * b + 16] = 1
            f[127] = 1
        out += [_edge("d-n7-weaker", 7, weaker, 8), _edge("d-n7-all-but-last", 7, all_but_last, 9), _edge("d-n7-half-tail", 7, half_and_tail, 10)]
        return {t.name: t for t in out}
    return _once("edge", make)


def is_up_set(frozen):
    """Is the unfrozen set closed upwards in the bitwise order: no unfrozen i with a frozen i | (1 << k)?"""
    frozen = np.asarray(frozen, bool)
    i = np.arange(len(frozen))
    k = 1
    while k < len(frozen):
        if (~frozen[i] & frozen[i | k]).any():
            return False
        k <<= 1
    return True


def octet_patterns(frozen):
    return (np.asarray(frozen, np.int64).reshape(-1, 8) << np.arange(8)).sum(axis=1)


def quad_patterns(frozen):
    return (np.asarray(frozen, np.int64).reshape(-1, 4) << np.arange(4)).sum(axis=1)


# ---- the SC pass and the guard model, vectorised over rows -----------------------------------------------------------------------

def sc_pass(code, llr):
    """flip_numpy.sc_pass without flips: (u [T, N], leaf [T, N])."""
    import flip_numpy as F
    return F.sc_pass(code, llr)


def margins(code, llr, u):
    """guard_numpy.l1_margins over rows llr [T, N] along decisions u [T, N] -> (prod [T], fsum [T], zero [T], win [T]: the smallest
    distance from 40 over the f-nodes of the pass). tests/test_mask_cases.py pins it to l1_margins row by row."""
    llr, u = np.asarray(llr, np.float64), np.asarray(u, np.uint8)
    T = len(llr)
    prod, fsum, zero, win = np.ones(T), np.zeros(T), np.zeros(T, bool), np.full(T, np.inf)

    def rec(a, lo):
        nonlocal prod, fsum, zero, win
        size = a.shape[1]
        fz = code.frozen[lo:lo + size]
        if fz.all():
            fsum = np.maximum(fsum, np.abs(a).sum(axis=1))
        if not fz.any():
            prod = np.minimum(prod, np.prod(np.tanh(np.abs(a) / 2), axis=1))
            zero = zero | (a == 0).any(axis=1)
        if size == 1:
            return u[:, lo:lo + 1]
        x, y = a[:, 0::2], a[:, 1::2]
        win = np.minimum(win, np.abs(np.maximum(np.abs(x), np.abs(y)) - 40.0).min(axis=1))
        xl = rec(S.f_node(x, y), lo)
        xr = rec(S.g_node(x, y, xl), lo + size // 2)
        out = np.empty((T, size), np.uint8)
        out[:, 0::2], out[:, 1::2] = xl ^ xr, xr
        return out
    rec(llr, 0)
    return prod, fsum, zero, win


class Rows:
    """The 2 x 48 rows of a code: llr [96, N], sent [96, K], the SC pass (u, leaf), the model's margins, keep_l1 / keep_list (bool
    [96]: the rows the list-size-1 kernels / the list kernels are compared on) and the oracle's list-size-1 bits."""

    def __init__(self, tab):
        o, code = tab.oracle(), S.Code(tab)
        got = [o.synth_llr(tab.seed, 0, B_POINT, o.snr_sqrt_linear(e)) for e in EBNO]
        self.llr = np.concatenate([g[0] for g in got])
        self.sent = np.concatenate([g[1] for g in got])
        self.llr.setflags(write=False)
        self.code = code
        self.u, self.leaf = sc_pass(code, self.llr)
        self.prod, self.fsum, self.zero, self.win = margins(code, self.llr, self.u)
        bad_in = np.array([G.input_guard(r) for r in self.llr])
        tiny = np.array([G.row_tiny(r) for r in self.llr])
        first = np.array([G.first_descent(r).min() for r in self.llr])
        self.keep_list = ~bad_in & ~tiny & (first >= WINDOW) & (self.win >= WINDOW)
        self.keep_l1 = ~bad_in & (self.win >= WINDOW) & (self.prod >= PROD_MIN) & (self.fsum <= FSUM_MAX) & ~self.zero
        self.bits_l1 = o.decode_scl_llr(self.llr, 1)
        self.err_l1 = (self.bits_l1 != self.sent).any(axis=1)


def rows(tab):
    return _once(("rows", tab.name), lambda: Rows(tab))


# ---- SC-Flip and SCAN: CRC variants ---------------------------------------------------------------------------------------------------

def soft_codes():
    """The CRC variants (crc = 8) the LDS-capped families are compared on: the n = 10 octet-pattern codes, edge masks (b) and (c)."""
    e = edge_masks()
    return _once("soft", lambda: [t.with_crc() for t in octet_codes(10)] +
                 [e[k].with_crc() for k in e if k.startswith(("b-", "c-"))])


def _drawn(tab):
    def make():
        o = tab.oracle()
        got = [o.synth_llr(tab.seed, 0, B_POINT, o.snr_sqrt_linear(e)) for e in EBNO]
        return np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
    return _once(("drawn", tab.name), make)


def _balanced(good, count):
    """`count` True entries: the first count / 2 of the first Eb/N0 point (fewer if it has fewer), the rest from the second."""
    lo = np.flatnonzero(good[:B_POINT])[:count // 2]
    return np.concatenate([lo, B_POINT + np.flatnonzero(good[B_POINT:])[:count - len(lo)]])


def flip_rows(tab):
    """FLIP_ROWS rows on which flip_numpy's margins hold for pass 0 at max(FLIP_T) flips: (llr, sent)."""
    import flip_numpy as F

    def make():
        code = S.Code(tab)
        llr, sent = _drawn(tab)
        _, leaf = F.sc_pass(code, llr)
        m = np.sort(np.abs(leaf[:, code.frozen == 0]), axis=1)
        head = m[:, :F.t_eff(code, max(FLIP_T)) + 1]
        gap = (np.diff(head, axis=1) / np.maximum(head[:, 1:], 1e-300)).min(axis=1)
        idx = _balanced((gap >= 10 * F.MARGIN) & (m[:, 0] >= 10 * F.MARGIN), FLIP_ROWS)
        return llr[idx], sent[idx]
    return _once(("flip", tab.name), make)


def scan_rows(tab, margin=None):
    """(the first SCAN_ROWS drawn rows as they come: min-sum; SCAN_ROWS rows on which no unfrozen leaf of the exact model comes below
    SCAN_MARGIN in any of 4 iterations — scan_numpy.clean_rows' rule: exact arithmetic)."""
    import scan_numpy as M
    margin = SCAN_MARGIN if margin is None else margin

    def make():
        code = S.Code(tab)
        llr, _ = _drawn(tab)
        good = M.row_margins(code, M.decode(code, llr, max(M.ITERS), check=False)) >= margin
        return llr[:SCAN_ROWS], llr[_balanced(good, SCAN_ROWS)]
    return _once(("scan", tab.name, margin), make)


def measure_scan_tol(draws=(0,), codes=None, tol=None):
    """scan_numpy.measure_tol on these codes: the largest deviation of a finite soft output between the exact model and the model
    with perturbed exp / log results, over the exact-mode rows of `codes` (default: all of soft_codes()) at 4 iterations."""
    import scan_numpy as M
    worst = 0.0
    for seed in draws:
        rng = np.random.default_rng(seed)
        for tab in (soft_codes() if codes is None else codes):
            code = S.Code(tab)
            llr = scan_rows(tab, None if tol is None else 100 * tol)[1]
            a = M.decode(code, llr, max(M.ITERS), check=False)
            b = M.decode(code, llr, max(M.ITERS), check=False, f=M.perturbed(rng))
            for name in ("info_llr", "ext"):
                fin = np.isfinite(a[name])
                assert (np.isfinite(b[name]) == fin).all()
                worst = max(worst, float(np.abs(a[name][fin] - b[name][fin]).max()))
    return worst


# ---- the whole list at N = 128 ---------------------------------------------------------------------------------------------------------

def scan_codes():
    """soft_codes() and the CRC variants of edge masks (a), whose frozen tails fix coded bits (ext = +inf)."""
    e = edge_masks()
    return _once("scan_codes", lambda: soft_codes() + [e["a-last-leaf"].with_crc(), e["a-last-quad"].with_crc()])


def adaptive_case():
    """The code of the adaptive comparison: the CRC variant of the first N = 128 mask."""
    return _once("adaptive", lambda: n128_masks()[0].with_crc())


def n128_masks():
    e = edge_masks()
    return [e[k] for k in e if k.startswith("d-")]


def list_rows(tab, Ls):
    """The first LIST_N128_ROWS drawn rows of an N = 128 mask and, per list size of Ls, scl_list's survivors (None where it raises
    TieError: the row is excluded for every list size) -> (llr, sent, {L: [rows]}, kept indices)."""
    def make():
        code = S.Code(tab)
        llr, sent = _drawn(tab)
        idx = np.concatenate([np.arange(LIST_N128_ROWS // 2), B_POINT + np.arange(LIST_N128_ROWS // 2)])
        llr, sent = llr[idx], sent[idx]
        lists, ok = {L: [] for L in Ls}, np.ones(len(llr), bool)
        for i in range(len(llr)):
            for L in Ls:
                try:
                    lists[L].append(S.scl_list(code, llr[i], L))
                except S.TieError:
                    lists[L].append(None)
                    ok[i] = False
        return llr, sent, lists, np.flatnonzero(ok)
    return _once(("list", tab.name, tuple(Ls)), make)
