"""The criteria by which the fast decode kernels hand a codeword to the fallback pass, stated once in plain numpy (DESIGN.md "Which
rows take the fallback pass"), the plants that put a row on either side of each of them, and the table of inputs that
tests/test_guard_model.py (CPU: the conditions on the inputs) and tests/test_gpu_fallback_rows.py (GPU: the fallback set of every
family and variant) share.

Nothing here knows of lanes, layouts or schedules: the arithmetic is tests/scl_list_numpy.py's (f_node, g_node), rows are in natural
order (the top layer combines the channel positions 2q and 2q + 1), decisions u in decoding order.
"""
import numpy as np

from scl_list_numpy import f_node, g_node


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
B = 70                                     # ragged against 8 rows per wave, 32 per flag word and 64
B_LARGE = 40                               # the large code
ORDINARY_B = 20                            # the batch between two planted ones ("flags left behind")
DELTAS_IN = (0.0, 5e-11, -5e-11)           # inside both windows
DELTAS_OUT = (1e-9, -1e-9)                 # outside both


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


def planted(base, batch, L, fmt="f64"):
    """A copy of the base rows [b][N] (doubles) in the element format with the batch's plants applied -> (rows, the sorted rows that
    the families of list size L hand to the fallback pass)."""
    rows = narrow(base, fmt).copy()
    want = []
    for r, pl in zip(planted_positions(rows.shape[0]), batch):
        if pl.flagged(L) is None:
            continue
        pl.apply(rows[r])
        if pl.flagged(L):
            want.append(r)
    return rows, np.array(sorted(want), np.uint32)
