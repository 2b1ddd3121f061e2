"""The criteria by which the fast decode kernels hand a codeword to the fallback pass, stated once in plain numpy (DESIGN.md "Which
rows take the fallback pass"), the plants that put a row on either side of each of them, and the table of inputs that
tests/test_guard_model.py (CPU: the conditions on the inputs) and tests/test_gpu_fallback_rows.py (GPU: the fallback set of every
family and variant) share.

Nothing here knows of lanes, layouts or schedules: the arithmetic is tests/scl_list_numpy.py's (f_node, g_node), rows are in natural
order (the top layer combines the channel positions 2q and 2q + 1), decisions u in decoding order.
"""
import numpy as np

from scl_list_numpy import TieError, crc_ok, f_node, g_node, leaf_cost, split


# ---- the criteria ---------------------------------------------------------------------------------------------------------------

def input_guard(row):
    """Any element non-finite or |x| < 1e-9, of the values AS WIDENED to double from their element format: float32(1e-9) widens to
    9.9999997e-10 and is flagged, the double 1e-9 is not."""
    a = np.abs(widen(row))
    return bool((~np.isfinite(a) | (a < 1e-9)).any())


def row_tiny(row):
    """No element with |x| >= 0.1 (the list families only; the list-size-1 kernels have no such criterion)."""
    return not bool((np.abs(widen(row)) >= 0.1).any())


def first_descent(row):
    """Layers 1 .. n of the all-f chain, which every path shares before any decision: per layer min | max(|a|, |b|) - 40 | over the
    layer's nodes -> [n]."""
    a = widen(row)
    out = []
    while a.size > 1:
        x, y = a[0::2], a[1::2]
        out.append(np.abs(np.maximum(np.abs(x), np.abs(y)) - 40.0).min())
        a = f_node(x, y)
    return np.array(out)


def sc_decisions(code, row):
    """The successive-cancellation decisions u [N] of a row (0 at frozen leaves and where the leaf is not negative)."""
    def rec(a, lo):
        S = a.size
        if S == 1:
            u = np.uint8(0 if code.frozen[lo] else a[0] < 0)
            return np.array([u], np.uint8), np.array([u], np.uint8)
        ul, xl = rec(f_node(a[0::2], a[1::2]), lo)
        ur, xr = rec(g_node(a[0::2], a[1::2], xl), lo + S // 2)
        x = np.empty(S, np.uint8)
        x[0::2], x[1::2] = xl ^ xr, xr
        return np.concatenate([ul, ur]), x
    return rec(widen(row), 0)[0]


def l1_margins(code, row, u):
    """An SC pass along the decisions u over EVERY node of the tree (so that the answer does not depend on where a kernel's schedule
    prunes) -> (the smallest prod tanh(|x_i| / 2) over the root values of any all-unfrozen node (the kernels flag below 1e-8),
    the largest sum of root |x| over any all-frozen node (they flag above 690), whether an all-unfrozen node has an exact-zero
    root value, the distances | max(|a|, |b|) - 40 | of every f-node of the pass as one array)."""
    u = np.asarray(u, np.uint8)
    prod, fsum, zero, win = [1.0], [0.0], [False], []

    def rec(a, lo):
        S = a.size
        fz = code.frozen[lo:lo + S]
        if fz.all():
            fsum[0] = max(fsum[0], float(np.abs(a).sum()))
        if not fz.any():
            prod[0] = min(prod[0], float(np.prod(np.tanh(np.abs(a) / 2))))
            zero[0] = zero[0] or bool((a == 0).any())
        if S == 1:
            return u[lo:lo + 1]
        x, y = a[0::2], a[1::2]
        win.append(np.abs(np.maximum(np.abs(x), np.abs(y)) - 40.0))
        xl = rec(f_node(x, y), lo)
        xr = rec(g_node(x, y, xl), lo + S // 2)
        out = np.empty(S, np.uint8)
        out[0::2], out[1::2] = xl ^ xr, xr
        return out
    rec(widen(row), 0)
    return prod[0], fsum[0], zero[0], np.concatenate(win)


def pruned_nodes(code):
    """The nodes whose input the PRUNED list-size-1 pass computes (the schedule of derive_tables: an all-frozen node decides zeros,
    an all-unfrozen one decides at its root, only a MIXED node descends): the root and both children of every mixed node, as
    (depth, index) — the node covers the leaves index * (N >> depth) onwards. The f-node that fills the input of (d + 1, 2 i) is
    evaluated by those kernels if and only if (d + 1, 2 i) is in this set, that is if (d, i) is mixed."""
    out = {(0, 0)}

    def rec(d, i):
        S = code.N >> d
        fz = code.frozen[i * S:(i + 1) * S]
        if S > 1 and fz.any() and not fz.all():
            out.update(((d + 1, 2 * i), (d + 1, 2 * i + 1)))
            rec(d + 1, 2 * i)
            rec(d + 1, 2 * i + 1)
    rec(0, 0)
    return out


def node_index(path):
    """The index of the node reached from the root by the f (0) / g (1) steps of `path`, top layer first."""
    i = 0
    for bit in path:
        i = 2 * i + int(bit)
    return i


# ---- the list walk ----------------------------------------------------------------------------------------------------------------

def weak_mask(code):
    """derive_tables' weak leaves, restated: the erasure probability z of a BEC(1/2) and its complement om = 1 - z (tracked as such:
    z itself rounds to 1) through the n layers, top layer first — f: z' = 2 z - z^2, om' = om^2; g: z' = z^2, om' = om (1 + z) —;
    an unfrozen leaf with om < 1e-3 is weak -> bool [N]."""
    z, om = np.array([0.5]), np.array([0.5])
    for _ in range(code.n):
        z2, om2 = np.empty(2 * z.size), np.empty(2 * z.size)
        z2[0::2], om2[0::2] = 2 * z - z * z, om * om
        z2[1::2], om2[1::2] = z * z, om * (1.0 + z)
        z, om = z2, om2
    return (code.frozen == 0) & (om < 1e-3)


class ListMargins:
    """What list_margins returns. visits: a list of (layer, phi, dist [paths][S]) — one entry per f-visit of the walk, dist[p][j] =
    | max(|a|, |b|) - 40 | of the f-node that gives element j of that layer for the living path p (in natural order: from the elements
    2 j and 2 j + 1 of the layer above). hyp (tables=True only): [4][N / 4], the same distance for the four hypotheses of the layer-2
    f-nodes at phi = N / 2, variant ua + 2 ub. weak: {phi: the smallest |leaf LLR| over the active paths} for every weak unfrozen
    leaf. u, info: the winner's decisions (findMostProbablePath)."""

    def __init__(self):
        self.visits, self.hyp, self.weak, self.u, self.info = [], None, {}, None, None

    def near(self, tol, hyp=True):
        """The evaluated f-nodes closer than tol, sorted by distance -> a list of (dist, layer, element, phi); a hypothesis of the
        table build is reported at layer 2, phi = N / 2 like the living paths' node it stands for (once per variant)."""
        out = []
        for lam, phi, d in self.visits:
            for p, j in zip(*np.nonzero(d < tol)):
                out.append((float(d[p, j]), lam, int(j), phi))
        if hyp and self.hyp is not None:
            for v, j in zip(*np.nonzero(self.hyp < tol)):
                out.append((float(self.hyp[v, j]), 2, int(j), -1 - int(v)))
        return sorted(set(out))

    def min_weak(self):
        return min(self.weak.values()) if self.weak else np.inf


def list_margins(code, row, L, tables=False):
    """A list-of-L walk over a row in the arithmetic and with the fork ranking of scl_list_numpy.scl_list (recursivelyCalcLLR from
    lam_top only, the L smallest of the 2 L fork metrics, TieError where the tie rule would decide), at any N, that records what the
    exp-domain list kernels guard: every f-node evaluated for a living path, and the leaf LLRs of the weak unfrozen leaves.

    The walk evaluates EVERY node; the kernels skip the f-nodes inside an aligned all-frozen block of 4 or 8 leaves (the rate-0
    schedule: the block's root values are all they need) — a subset, so a row that keeps its distance here keeps it there, and a plant
    must sit at an f-node whose output feeds a leaf that is not frozen (tests/test_guard_model.py asserts that).

    tables=True adds what the table build of the list of 32 evaluates at phi = N / 2 (polar_scl_visits.inc, kind 2), in the place of
    the paths' own visits of layers 1 and 2 there: per element j of layer 2 (j < N / 4) and per pair of partial-sum bits (ua, ub),
    f(g(c[4 j], c[4 j + 1], ua), g(c[4 j + 2], c[4 j + 3], ub)) of the channel values c — all four combinations of every element, by
    all lanes of the codeword, whether or not a living path holds that pair of bits. (Kinds 1 and 3, at N / 4 and 3 N / 4, build
    g-nodes only; layer 3 and below are visited per path from the table's values, which are the values of this walk.)"""
    n, N = code.n, code.N
    out = ListMargins()
    c = widen(row).reshape(1, N)
    weak = weak_mask(code)
    A = [c] + [np.zeros((1, N >> lam)) for lam in range(1, n + 1)]
    CL = [np.zeros((1, N >> lam), np.uint8) for lam in range(n + 1)]
    CR = [np.zeros((1, N >> lam), np.uint8) for lam in range(n + 1)]
    U = np.zeros((1, N), np.uint8)
    pm = np.zeros(1)
    if tables and n >= 2:
        a4 = c[0].reshape(-1, 4)
        hyp = np.empty((4, N // 4))
        for v in range(4):
            ua, ub = np.uint8(v & 1), np.uint8(v >> 1)
            x, y = g_node(a4[:, 0], a4[:, 1], ua), g_node(a4[:, 2], a4[:, 3], ub)
            hyp[v] = np.abs(np.maximum(np.abs(x), np.abs(y)) - 40.0)
        out.hyp = hyp
    for phi in range(N):
        lam_top = 1 if phi == 0 else n - ((phi & -phi).bit_length() - 1)
        for lam in range(lam_top, n + 1):
            a, b = A[lam - 1][:, 0::2], A[lam - 1][:, 1::2]
            if (phi >> (n - lam)) & 1:
                A[lam] = g_node(a, b, CL[lam])
            else:
                d = np.abs(np.maximum(np.abs(a), np.abs(b)) - 40.0)
                out.visits.append((lam, phi, np.broadcast_to(d, (len(pm), d.shape[1])) if d.shape[0] != len(pm) else d))
                A[lam] = f_node(a, b)
        v = A[n][:, 0]
        if code.frozen[phi]:
            pm = pm + leaf_cost(-v)
            bit = np.zeros(len(pm), np.uint8)
        else:
            if weak[phi]:
                out.weak[phi] = float(np.abs(v).min())
            na = len(pm)
            m = np.concatenate([pm + leaf_cost(-v), pm + leaf_cost(v)])
            keep = np.argsort(m, kind="stable")
            if 2 * na > L:
                if m[keep[L - 1]] == m[keep[L]]:
                    raise TieError("fork metrics %d and %d are equal at leaf %d" % (L, L + 1, phi))
                keep = np.sort(keep[:L])
            src, bit = keep % na, (keep // na).astype(np.uint8)
            A = [x[src] if x.shape[0] == na and i else x for i, x in enumerate(A)]
            CL, CR, U, pm = [x[src] for x in CL], [x[src] for x in CR], U[src], m[keep]
        U[:, phi] = bit
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
    if len(set(pm.tolist())) != len(pm):
        raise TieError("two survivors end with equal metrics")
    info, check = split(code, U)
    ok = crc_ok(code, info, check)
    cand = np.nonzero(ok)[0] if ok.any() else np.arange(len(pm))
    w = cand[np.argmin(pm[cand])]
    out.u, out.info = U[w].copy(), info[w].copy()
    return out


# ---- element formats ------------------------------------------------------------------------------------------------------------

def widen(row):
    """The values of a row as doubles: float64 / float32 / float16 arrays as they are, uint16 arrays as bfloat16 patterns."""
    a = np.asarray(row)
    if a.dtype == np.uint16:
        return (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return a.astype(np.float64)


def narrow(rows, fmt):
    """Rows of doubles in an element format ("f64", "f32", "f16"; "bf16": the patterns, by truncation of the float32)."""
    if fmt == "bf16":
        return (np.ascontiguousarray(rows, np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return np.ascontiguousarray(rows, {"f64": np.float64, "f32": np.float32, "f16": np.float16}[fmt])


def _set(row, col, value):
    """value (a double) into row[col] in the row's element format."""
    if row.dtype == np.uint16:
        row[col] = (np.array([value], np.float32).view(np.uint32) >> 16).astype(np.uint16)[0]
    else:
        row[col] = value


# ---- the plants -----------------------------------------------------------------------------------------------------------------

def plant_window(row, layer, block, delta, partner=45.0, sign=1.0):
    """Rewrites the 2^layer consecutive channel elements from block * 2^layer on: element 0 becomes sign * (40 + delta), element
    2^(layer-1) keeps its sign at magnitude 3.0, every other element of the block keeps its sign at magnitude `partner`. The top
    layer combines (2q, 2q + 1), so every node above `layer` sees max |x| = partner >= 40 and takes the min-sum branch, which copies
    the smaller magnitude exactly (in exp-domain form: a copy of E); the node at `layer` sees max |x| = 40 + delta. (The partner is 45
    and not 600: sums of 600s would trip the list-size-1 kernels' all-frozen bound of 690.)"""
    S = 1 << layer
    lo = block * S
    sg = np.where(np.signbit(row[lo:lo + S]), -1.0, 1.0)
    row[lo:lo + S] = sg * partner
    row[lo] = sign * (40.0 + delta)
    row[lo + S // 2] = sg[S // 2] * 3.0
    return row


def plant_scaled(row, largest):
    """The row scaled so that its largest magnitude is exactly `largest`."""
    k = int(np.abs(row).argmax())
    row *= largest / abs(row[k])
    row[k] = np.copysign(largest, row[k])
    return row


def encode(u):
    """The codeword x [N] (natural order) of decisions u [N] (decoding order): x[0::2] = x_left ^ x_right, x[1::2] = x_right."""
    u = np.asarray(u, np.uint8)
    if u.size == 1:
        return u.copy()
    h = u.size // 2
    xl, xr = encode(u[:h]), encode(u[h:])
    x = np.empty(u.size, np.uint8)
    x[0::2], x[1::2] = xl ^ xr, xr
    return x


PARTNER = 45.0


def plant_node(row, code, path, element, value, u=None, salt=0):
    """Rewrites the 2^d channel elements under ONE element of the input of the node that the d steps of `path` (0: f, 1: g, top layer
    first) reach, so that the reference's own arithmetic delivers exactly `value` there on the path whose earlier decisions are u
    (None: the row's own successive-cancellation decisions, taken before anything is rewritten).

    The signs of the block follow the codeword x = encode(u), whose partial codewords at the nodes along the path are the partial sums
    that path holds, so every g-step on it ADDS magnitudes. Upwards from the element: at an f-step the value's sibling is a partner of
    magnitude 45 to 49 (or up to 4 above the value's own, if that is larger), so the f-node above takes the min-sum branch and copies the smaller magnitude
    exactly (in exp-domain form: a copy of E); at a g-step a magnitude D is split into D/2 + 0.25 and what is left of D (D/2 + D/8
    below 2, D/2 + 21 for a partner), both exact and unequal — a path that holds the other partial sum sees their difference, not a zero. A value whose sign
    is not the codeword's flips the signs of its whole chain: of both summands at a g-step (the left sibling subtree, which sees their
    product, decides as before), of the value's side alone at an f-step."""
    N, d = code.N, len(path)
    if u is None:
        u = sc_decisions(code, row)
    xs = [encode(u)]
    for bit in path:
        x = xs[-1]
        xs.append(x[1::2] if bit else x[0::2] ^ x[1::2])
    sg = 1.0 - 2.0 * xs[d][element]

    def deliver(mag, flip, k, e):
        if k == 0:
            _set(row, e, flip * (1.0 - 2.0 * xs[0][e]) * mag)
        elif path[k - 1] == 0:
            deliver(mag, flip, k - 1, 2 * e)
            # (no two partners alike: a block of equal magnitudes makes fork metrics of different paths EQUAL, which is a TieError)
            deliver(max(PARTNER, mag) + 4.0 * (((2 * e + 1) * 0.6180339887498949 + k * 0.137 + salt * 0.377) % 1.0), 1.0, k - 1, 2 * e + 1)
        else:
            # (a PARTNER is split 42 apart: under the other partial sum it stays a partner — the table build pairs every value with
            # its sibling under all four pairs of partial sums, and (40 + delta, 0.5) would be a second f-node in the window)
            a = mag / 2 + (21.0 + ((e * 0.7548776662466927 + k * 0.311) % 1.0) if mag >= PARTNER else 0.25 if mag >= 2 else mag / 8)
            deliver(a, flip, k - 1, 2 * e)
            deliver(mag - a, flip, k - 1, 2 * e + 1)
    deliver(abs(value), 1.0 if np.copysign(1.0, value) == sg else -1.0, d, element)
    return row


def plant_pair(row, code, path, j, delta, sign=1.0, salt=0, twin=3.0):
    """The pair (2 j, 2 j + 1) of the input of the node at `path`: sign * (40 + delta) and its twin at magnitude 3.0 in the codeword's
    sign, as plant_window's. The f-node that gives element j of layer len(path) + 1 then sees max |x| = 40 + delta. (`twin`: another
    magnitude below 40 for the twin — the f-node's output, which is what the leaves below it see.)"""
    u = sc_decisions(code, row)
    x = encode(u)
    for bit in path:
        x = x[1::2] if bit else x[0::2] ^ x[1::2]
    plant_node(row, code, path, 2 * j, sign * (40.0 + delta), u, salt)
    plant_node(row, code, path, 2 * j + 1, (1.0 - 2.0 * x[2 * j + 1]) * twin, u, salt)
    return row


def plant_hypothesis(row, code, j, delta, sign=1.0):
    """The channel elements 4 j .. 4 j + 3 such that element j of layer 2 comes within delta of the window at phi = N / 2 ONLY under a
    partial sum that no path holds: (c0, c1) = (23, 63 + delta) in the codeword's signs — the first half of the codeword sees
    f = +-23 and every living path holds the codeword's ua, g = 86 + delta; the other ua gives +-(40 + delta), exactly (both numbers
    are multiples of the same ulp) —, (c2, c3) = (1, 2): 3 or 1 under either ub. `sign` = -1 swaps the magnitudes of c0 and c1."""
    x = encode(sc_decisions(code, row))
    s = 1.0 - 2.0 * x[4 * j:4 * j + 4]
    big = (40.0 + delta) + 23.0
    mags = (23.0, big, 1.0, 2.0) if sign > 0 else (big, 23.0, 1.0, 2.0)
    for k in range(4):
        _set(row, 4 * j + k, s[k] * mags[k])
    return row


# the two window forms of the exp-domain f-node, restated: E is the smaller of the node's two stored values
E40 = 4.248354255291589e-18


def in_wave_window(E):
    """f_node_e: E in (e^-40 (1 - 1e-10), e^-40 (1 + 1e-10)]."""
    return E40 * (1.0 - 1e-10) < E <= E40 * (1.0 + 1e-10)


def in_lane_window(E):
    """f_node_e_acc and the flag at the codeword's end: | E - e^-40 (1 + 1e-10) | <= e^-40 * 2.0000001e-10."""
    return abs(E - E40 * (1.0 + 1e-10)) <= E40 * 2.0000001e-10


# ---- the shared table -----------------------------------------------------------------------------------------------------------
EPS = 0.32
EBNO = 1.5
# (n, K, crc) -> the seed of its rows. Moved on the CPU (tests/test_guard_model.py), never after a GPU result: (9, 256, 8) from 7102 —
# one ordinary row came within 6e-4 of |x| = 40 at a node of its list-size-1 pass once rounded to 16 bits; 7110 and 7111 likewise
CODES = {(7, 64, 8): 7101, (9, 256, 8): 7112, (11, 1024, 16): 7103}
# (n, K, crc) -> the trials of that seed that are NOT rows: one of their f-nodes below the first descent comes within 1e-3 of |x| = 40
# for a living path of a list decode (list_margins; 2, 4, 8 on the first code, 32 on the last) — with some 1e7 such nodes per
# batch of the large code, six of the first forty trials do (the nearest at 9.5e-6) and trial 41 of those that fill the batch up, so no seed clears a whole batch there and the
# rows are the first trials that keep their distance. Found on the CPU, asserted by tests/test_guard_model.py.
SKIPPED = {(7, 64, 8): (12,), (9, 256, 8): (), (11, 1024, 16): (11, 12, 13, 27, 29, 30, 41)}
B = 70                                     # ragged against 8 rows per wave, 32 per flag word and 64
B_LARGE = 40                               # the large code
ORDINARY_B = 20                            # the batch between two planted ones ("flags left behind")
DELTAS_IN = (0.0, 5e-11, -5e-11)           # inside both windows
DELTAS_OUT = (1e-9, -1e-9)                 # outside both


def base_rows(o, key):
    """The ordinary rows [b][N] of a code of the table from its oracle object: the trials 0, 1, ... of its seed at EBNO without the
    SKIPPED ones, read-only."""
    b = B_LARGE if key[0] == 11 else B
    trials = [t for t in range(b + len(SKIPPED[key])) if t not in SKIPPED[key]]
    assert len(trials) == b
    llr = o.synth_llr_trials(CODES[key], trials, o.snr_sqrt_linear(EBNO))[0]
    llr.setflags(write=False)
    return llr


def planted_positions(b):
    """Rows 0, 31, 32, 33 and the last one: both sides of a flag word's edge, two neighbours, the ragged tail. (Batches of fewer
    rows, for a capped grid of three waves: 0, 3, 4, 5 and the last one — each wave meets a planted row and ordinary ones after it.)"""
    return (0, 31, 32, 33, b - 1) if b > 34 else (0, 3, 4, 5, b - 1)


def window_sites(N):
    """(layer, block): layer 1 at blocks 0, N/2 - 1 and one in between, layer 2 at block 0 and at the last block."""
    return ((1, 0), (1, N // 2 - 1), (1, N // 4 + 3), (2, 0), (2, N // 4 - 1))


class Plant:
    """One planted row: its name, whether the list families / the list-size-1 families flag it (None: the row is left ordinary
    there), what it rests on ("input", "tiny", "window" or "control") and the function that rewrites the row in place."""

    def __init__(self, name, flag_list, flag_l1, kind, apply):
        self.name, self.flag_list, self.flag_l1, self.kind, self.apply = name, flag_list, flag_l1, kind, apply

    def flagged(self, L):
        return self.flag_l1 if L == 1 else self.flag_list

    def __repr__(self):
        return self.name


def _at(col, value):
    return lambda row: _set(row, col % row.size, value)


def _window(site, delta, sign):
    return lambda row: plant_window(row, site[0], site[1], delta, sign=sign)


def batches(N, fmt="f64"):
    """The planted batches of a code and an element format: a list of tuples of five Plants, for planted_positions() in turn.
    f64: two batches of input plants (with the tiny row and its control: list families only) and ten of window plants — every site
    with every delta and both signs, every batch holding all five sites and all five deltas. f32 adds float32(1e-9); f16 and bf16
    plant +-0 and +-inf only, f16 also its smallest subnormal as a control."""
    zero = Plant("0.0 in column 0", True, True, "input", _at(0, 0.0))
    nzero = Plant("-0.0 in the last column", True, True, "input", _at(-1, -0.0))
    pinf = Plant("+inf", True, True, "input", _at(5, np.inf))
    ninf = Plant("-inf", True, True, "input", _at(N // 2 + 1, -np.inf))
    if fmt in ("f16", "bf16"):
        last = Plant("smallest subnormal", False, False, "control", _at(7, 2.0 ** -24)) if fmt == "f16" else \
            Plant("ordinary row", False, False, "control", lambda row: None)
        return [(zero, pinf, ninf, nzero, last)]
    below = Plant("9.99e-10", True, True, "input", _at(N - 2, 9.99e-10))
    at = Plant("1e-9 exactly", False, False, "control", _at(3, 1e-9))
    above = Plant("1.0000001e-9", False, False, "control", _at(N // 2, -1.0000001e-9))
    tiny = Plant("largest magnitude 0.09", True, None, "tiny", lambda row: plant_scaled(row, 0.09))
    sized = Plant("largest magnitude 0.1", False, None, "control", lambda row: plant_scaled(row, 0.1))
    if fmt == "f32":
        f32 = Plant("float32(1e-9)", True, True, "input", _at(9, float(np.float32(1e-9))))
        return [(zero, nzero, above, below, pinf), (ninf, f32, tiny, sized, zero)]
    assert fmt == "f64"
    out = [(zero, nzero, at, below, pinf), (ninf, above, tiny, sized, zero)]
    sites, deltas = window_sites(N), DELTAS_IN + DELTAS_OUT
    for k in range(10):
        sign = 1.0 if k < 5 else -1.0
        row = []
        for p, site in enumerate(sites):
            d = deltas[(p + k) % 5]
            inside = d in DELTAS_IN
            row.append(Plant("window layer %d block %d delta %+g sign %+d" % (site[0], site[1], d, sign), inside, inside,
                             "window" if inside else "control", _window(site, d, sign)))
            row[-1].site, row[-1].delta = site, d
        out.append(tuple(row))
    return out


# ---- windows below g-branches (tests/test_gpu_guard_sites.py) -------------------------------------------------------------------------

def _mixed(code, d, i):
    S = code.N >> d
    fz = code.frozen[i * S:(i + 1) * S]
    return bool(fz.any() and not fz.all())


def _first_path(code, d, lead=()):
    """The first path of d steps after `lead`, fewest g-steps first (at least one in all) and then in numerical order, whose node
    is mixed and has a mixed left child: both the pruned list-size-1 pass and the list kernels evaluate the f-nodes on its input."""
    best = None
    for v in range(1 << d):
        path = tuple(lead) + tuple((v >> (d - 1 - k)) & 1 for k in range(d))
        if sum(path) == 0:
            continue
        i = node_index(path)
        if _mixed(code, len(path), i) and _mixed(code, len(path) + 1, 2 * i):
            key = (sum(path), v)
            if best is None or key < best[0]:
                best = (key, path)
    assert best is not None, (d, lead)
    return best[1]


def node_sites(code):
    """{name: (path, j)}: the f-nodes below at least one g-branch that carry the plants. Read against the list kernel at its default
    LDS size (layers of up to 8 elements in LDS): "hbm" — the node after f, g (phi = N / 4): its f-visit is layer 3, written to the
    HBM-scratch rows of the batch kernel out of the fused pass that starts with the g-visit of layer 2; "lds" — a node with an input
    of 8 elements: the f-visit reads and writes LDS layers (a stored layer of the one-codeword-per-wave form as well); "regs" — a node
    with an input of 4 elements: the one-codeword-per-wave form evaluates it on registers; "late" — the LAST node of the codeword
    (largest first leaf, then smallest) that is mixed with a mixed left child, beyond 3 N / 4; "table" — the node after one g
    (phi = N / 2), the f-visit of layer 2 that table mode replaces by its build. j: an element away from the node's edges."""
    n = code.n
    sites = {}
    sites["hbm"] = ((0, 1), 3)
    sites["gf"] = ((1, 0), code.N // 16 + 2)
    sites["gff"] = ((1, 0, 0), code.N // 32 - 1)
    sites["mid"] = (_first_path(code, n - 5), 6)
    sites["lds"] = (_first_path(code, n - 3), 1)
    sites["regs"] = (_first_path(code, n - 2), 1)
    late = None
    for d in range(2, n - 1):
        for i in range(3 << (d - 2), 1 << d):
            if _mixed(code, d, i) and _mixed(code, d + 1, 2 * i):
                key = (i * (code.N >> d), d)
                if late is None or key > late[0]:
                    late = (key, tuple((i >> (d - 1 - k)) & 1 for k in range(d)))
    assert late is not None
    sites["late"] = (late[1], 0)
    sites["table"] = ((1,), code.N // 8 + 5)
    for name, (path, j) in sites.items():
        assert 2 * j + 1 < (code.N >> len(path)), (name, path, j)
    return sites


# (block length, plant) -> the salt of its partners' magnitudes, where those of salt 0 lead a living path of the planted row to
# within 1e-3 of |x| = 40 at some OTHER node (the partners' magnitudes are free; tests/test_guard_model.py asserts the result)
SALTS = {(11, "window at lds gfgfgfff pair 1 delta +1e-09 sign +1"): 1, (11, "window at lds gfgfgfff pair 1 delta +1e-09 sign -1"): 1}


def _node_plant(code, name, site, delta, sign, hyp=False):
    inside = delta in DELTAS_IN
    path, j = site
    if hyp:
        pl = Plant("hypothesis-only window, element %d delta %+g sign %+d" % (j, delta, sign), inside, None, "hyp" if inside else "control",
                   lambda row: plant_hypothesis(row, code, j, delta, sign))
    else:
        label = "window at %s %s pair %d delta %+g sign %+d" % (name, "".join("fg"[b] for b in path), j, delta, sign)
        salt = SALTS.get((code.n, label), 0)
        pl = Plant(label, inside, inside, "window" if inside else "control", lambda row: plant_pair(row, code, path, j, delta, sign, salt))
    pl.node, pl.delta, pl.site_name = (path, j), delta, name
    return pl


SITE_NAMES = ("hbm", "table", "gf", "gff", "mid", "lds", "regs", "late")


def node_batches(code, fmt="f64", names=SITE_NAMES, full=("hbm", "lds")):
    """The planted batches of the sites `names` of node_sites: every site with one plant inside the window and one control outside,
    five to a batch (the last batch filled up with further plants of the first site), then for each site of `full` one batch of all
    five deltas with sign + and one with sign -. -> a list of tuples of five Plants.

    f32, f16, bf16: |x| = 40 is the only planted magnitude those formats hold exactly (its chain of halves plus or minus a quarter
    as well, through three g-steps), so every other delta — the controls among them — is left out: batches of plants with delta 0
    alone, both signs, at all sites."""
    sites = node_sites(code)
    deltas = DELTAS_IN + DELTAS_OUT
    if fmt != "f64":
        flat = [_node_plant(code, name, sites[name], 0.0, 1.0 if k % 2 == 0 else -1.0) for k, name in enumerate(names)]
        while len(flat) % 5:
            k = len(flat)
            flat.append(_node_plant(code, names[k % len(names)], sites[names[k % len(names)]], 0.0, 1.0 if k % 2 else -1.0))
        return [tuple(flat[i:i + 5]) for i in range(0, len(flat), 5)]
    flat = []
    for k, name in enumerate(names):
        flat.append(_node_plant(code, name, sites[name], DELTAS_IN[k % 3], 1.0 if k % 2 == 0 else -1.0))
        flat.append(_node_plant(code, name, sites[name], DELTAS_OUT[k % 2], 1.0 if k % 2 == 0 else -1.0))
    k = 0
    while len(flat) % 5:
        flat.append(_node_plant(code, names[0], sites[names[0]], deltas[(k + 1) % 5], -1.0))
        k += 1
    out = [tuple(flat[i:i + 5]) for i in range(0, len(flat), 5)]
    for name in full:
        if name in names:
            for sign in (1.0, -1.0):
                out.append(tuple(_node_plant(code, name, sites[name], d, sign) for d in deltas))
    return out


def hypothesis_batch(code):
    """Table mode only: three plants whose window lies in a hypothesis that no path holds (flagged where the table build runs, not
    flagged where the paths visit layer 2 themselves: Plant.kind "hyp"), one control outside, and the living-path plant at "table"."""
    N = code.N
    t = node_sites(code)["table"]
    return (_node_plant(code, "table", ((1,), 2), 0.0, 1.0, hyp=True), _node_plant(code, "table", ((1,), N // 8 + 1), 1e-9, 1.0, hyp=True),
            _node_plant(code, "table", ((1,), N // 4 - 1), -5e-11, -1.0, hyp=True), _node_plant(code, "table", t, 5e-11, -1.0),
            _node_plant(code, "table", ((1,), 7), 5e-11, 1.0, hyp=True))


# ---- the weak-leaf guard ----------------------------------------------------------------------------------------------------------------
# A code with weak unfrozen leaves ((9, 505, 0.7, crc 0) of tests/test_gpu_fuzz.py), whose ORDINARY rows the guard often
# flags: the expected set is the model's (list_margins(...).min_weak() below WEAK_EDGE), recorded here and asserted against the model
# on the CPU. Seed, first trial and Eb/N0 were chosen on the CPU so that the model alone puts at least five ordinary rows on each
# side at every list size used and leaves none out (a row is left out of the set comparison when its smallest weak leaf lies in
# [0.9e-8, 1.1e-8] or one of its f-nodes comes within 1e-3 of the window): at 2 dB every row is flagged, at 6 dB none; seed 7202 at
# 5 dB has five flagged trials (8, 12, 13, 31, 68), and counting from trial 1 keeps them off the planted positions.
WEAK_CODE = (9, 505, 0.7, 0)
WEAK_SEED, WEAK_TRIAL0, WEAK_EBNO = 7202, 1, 5.0
WEAK_LS = (4, 8, 32)
WEAK_EDGE = 1.000000005e-8                 # the guard fires for E > 0.99999999, that is |x| < -log(0.99999999)
WEAK_FLAGGED = (7, 11, 12, 30, 67)         # the ordinary rows the model flags, at each of WEAK_LS
WEAK_LEFT_OUT = ()


def weak_rows(o):
    llr = o.synth_llr(WEAK_SEED, WEAK_TRIAL0, B, o.snr_sqrt_linear(WEAK_EBNO))[0]
    llr.setflags(write=False)
    return llr


def weak_batch(code):
    """Five plants of the LLR of leaf 0, a weak leaf that only f-steps reach: plant_node rewrites the whole row so that a min-sum
    chain delivers the planted value there — copies, so it is exact — and every other leaf sees a partner's magnitude. (A leaf below
    a g-step cannot be planted this way: the two summands of a value of 1e-8 are as small, and the f-branch beside them hands
    their product to the weak leaves before.) 5e-9 and 0.99e-8 are flagged, 1.01e-8 and 2e-8 are not. The list-size-1 families
    have no such guard: None."""
    def one(leaf, value):
        path = tuple((leaf >> (code.n - 1 - k)) & 1 for k in range(code.n))
        pl = Plant("weak leaf %d at %+g" % (leaf, value), abs(value) < WEAK_EDGE, None, "weak" if abs(value) < WEAK_EDGE else "control",
                   lambda row: plant_node(row, code, path, 0, value))
        pl.leaf, pl.value = leaf, value
        return pl
    return (one(0, 5e-9), one(0, 1.01e-8), one(0, 0.99e-8), one(0, -2e-8), one(0, -0.99e-8))


# ---- rate-1 quads and octets finished in one step (the list of 32) ---------------------------------------------------------------
# polar_scl_leaf.inc finishes a marked block of four unfrozen leaves in the step of its first leaf, and the second quad of a marked
# octet in the same step; the f-nodes in there keep their guard distance in a temporary that reaches the lane's own only on commit.
# Read against the continuation, for the octet that starts at leaf phi0 (the first quad's node q, the second quad's node q2):
#   "quad"     the last f-node of the first quad (leaf phi0 + 2): the pair on the input of q + g
#   "chain_w"  the two f-nodes on the second quad's input of 4 (they give its layer of 2): pair j of the input of q2
#   "chain_y"  the f-node of the second quad's first leaf (leaf phi0 + 4): the pair on the input of q2 + f
#   "chain_z"  its last f-node (leaf phi0 + 6): the pair on the input of q2 + g
# A block is finished in one step only if every later leaf of it passes the fast test in BOTH codewords of the wave (rows 2 w and
# 2 w + 1), so each wave that holds a plant gets the plant's control (or a second plant of the same block) as its other row, and the
# twin of the planted pair — the f-node's output, which a leaf of the block sees — is not 3.0 but a magnitude in the thirties: with 3.0
# the spread of the 32 path metrics exceeds the leaf and no block is finished in one step. Block, twin and salt of every row were
# searched on the CPU (no tie, no other f-node within 1e-3, the model of tests/r1_chain_model.py finishes the block in one step);
# tests/test_guard_model.py asserts the result.
R1_B = 14                                  # rows: waves (0, 1), (2, 3), (4, 5) and (12, 13) hold the plants
R1_L = 32
# (row, kind, phi0, pair, delta, sign, twin, salt)
R1_PLANTS = ((0, "quad", 452, 0, 0.0, 1.0, 39.0, 1), (1, "quad", 452, 0, 1e-9, 1.0, 39.0, 1),             # a quad outside any octet:
             (3, "chain_w", 480, 1, 5e-11, -1.0, 39.0, 0), (2, "chain_w", 480, 1, -1e-9, -1.0, 39.0, 0),   # no chain carries its distance
             (4, "chain_y", 496, 0, -5e-11, 1.0, 37.5, 0), (5, "chain_y", 496, 0, 1e-9, 1.0, 37.5, 0),
             (6, "chain_w", 480, 0, 5e-11, 1.0, 39.0, 0), (7, "chain_w", 480, 0, -1e-9, 1.0, 39.0, 3),
             (13, "chain_z", 504, 0, 0.0, -1.0, 37.5, 0), (12, "chain_z", 504, 0, -1e-9, -1.0, 37.5, 0))


def _bits(v, d):
    return tuple((v >> (d - 1 - k)) & 1 for k in range(d))


def r1_site(code, kind, phi0, j=0):
    """(path, pair) of the f-node `kind` of the octet that starts at leaf phi0 — for "quad" also of a quad outside an octet."""
    n = code.n
    assert phi0 % (4 if kind == "quad" else 8) == 0
    q2 = _bits(phi0 >> 3, n - 3) + (1,)
    return {"quad": (_bits(phi0 >> 2, n - 2) + (1,), 0), "chain_w": (q2, j), "chain_y": (q2 + (0,), 0), "chain_z": (q2 + (1,), 0)}[kind]


def r1_batch(code, base, plants=None):
    """The first R1_B base rows with R1_PLANTS applied -> (rows, the sorted rows planted inside the window, [(the wave's first row, the
    leaf the block starts at, "quad" or "chain": which commit carries the planted distance)] per wave with a plant, the plants as
    Plant objects per row)."""
    rows = np.array(base[:R1_B], np.float64)
    want, blocks, pls = [], [], {}
    for r, kind, phi0, j, delta, sign, twin, salt in (R1_PLANTS if plants is None else plants):
        path, j = r1_site(code, kind, phi0, j)
        plant_pair(rows[r], code, path, j, delta, sign, salt, twin)
        inside = delta in DELTAS_IN
        pl = Plant("window at %s of the block at leaf %d, pair %d delta %+g sign %+d" % (kind, phi0, j, delta, sign), inside, inside,
                   "window" if inside else "control", None)
        pl.node, pl.delta, pl.block = (path, j), delta, (r & ~1, phi0, "quad" if kind == "quad" else "chain")
        pls[r] = pl
        if inside:
            want.append(r)
        if pl.block not in blocks:
            blocks.append(pl.block)
    return rows, np.array(sorted(want), np.uint32), blocks, pls


def r1_wave(code, rows2, L=R1_L):
    """One wave (two consecutive codewords, every test ANDed over both) by the model of tests/r1_chain_model.py -> (the blocks
    finished in one step as a set of (first leaf, "quad" | "chain": the second quad of the octet finished in the same step), the
    leaf tests of the rows, for r1_chain_model.counts)."""
    import r1_chain_model
    import r1_model
    fr = np.asarray(code.frozen, np.uint8)
    tests = [r1_model.leaf_tests(fr, r, L) for r in rows2]
    finished = []
    r1_chain_model.counts(fr, rows2, L, tests=tests, finished=finished)
    return {(phi, kind) for _, phi, kind in finished}, tests


def planted(base, batch, L, fmt="f64", tables=True):
    """A copy of the base rows [b][N] (doubles) in the element format with the batch's plants applied -> (rows, the sorted rows that
    the families of list size L hand to the fallback pass). tables=False: a kernel that builds no tables — the plants of kind "hyp"
    are applied and NOT expected."""
    rows = narrow(base, fmt).copy()
    want = []
    for r, pl in zip(planted_positions(rows.shape[0]), batch):
        if pl.flagged(L) is None:
            continue
        pl.apply(rows[r])
        if pl.flagged(L) and (tables or pl.kind != "hyp"):
            want.append(r)
    return rows, np.array(sorted(want), np.uint32)
