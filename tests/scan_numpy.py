"""SCAN soft-output decoding (include/polar_amd.h polar_decode_scan_batch) restated in numpy, unpruned, vectorised over
rows: what the device is tested against, and the inputs and expected counts the CPU and the GPU tests share.

Layer 0 is the channel row, layer n the leaves in decoding order; node v of layer lam has N >> lam values and the children 2v, 2v + 1,
which pair its neighbouring elements. A leaf's B is +inf if frozen, else 0; every internal B is 0 before iteration 1. At a node with
values a (a0 = a[0::2], a1 = a[1::2]), depth first:
    L_left  = f(a0, a1 + B_right)        B_right: the previous iteration's
    L_right = f(a0, B_left) + a1
    B[0::2] = f(B_left, B_right + a1),   B[1::2] = f(B_left, a0) + B_right
f is scl_list_numpy.f_node (exact mode) or ms_node (min-sum). In min-sum mode every operation is a min, a sign or one addition of
doubles: the device must match bit for bit, on any row.

Exact mode. numpy's exp / log and the kernel's table-driven ones agree to about 1e-13 relative (scl_list_numpy.py, flip_numpy.py);
that concerns the exp / log branch of the f-node alone — its min-sum branch (an argument of 40 or more, an infinite one among them) is
a min and a sign on both sides. What the disagreement does to the outputs is MEASURED here, on the CPU, model against model
(measure_tol): every result of the exp / log branch moved by a random relative 1e-13 plus absolute 1e-15, the largest deviation of
any finite info_llr / ext entry over all the rows the exact-mode tests use at the largest `iters` they use them at. TOL is ten times
that (the perturbation is random, not worst-case). A row whose hard result could depend on TOL — an unfrozen leaf LLR below MARGIN =
100 TOL in magnitude at the end of any iteration — raises MarginError instead of being decoded.

Two things the measurement showed, and what the shared inputs do about them:
  * Small leaf LLRs are common, not rare. Iteration 1 gives a right child f(a0, 0) + a1 = a1 where its left sibling is all unfrozen,
    and the leaves below take f of many small values: of 64 plain rows at 1.5 dB 11 (n = 10) and 14 (n = 11) have an unfrozen leaf
    below 1e-7, some below 1e-14; rows scaled by 50 produce exact zeros (min-sum values cancel in the additions). No seed gives 64
    consecutive trials without one. The rows of an EXACT-mode test are therefore the first trials of its seed on which the model
    raises no MarginError (clean_rows) — chosen on the CPU, by the model alone. Min-sum mode needs no margin and is compared on the
    first 64 trials as they come (plain_rows), plain and scaled: the rows with zeros and near-zeros among them.
  * On rows scaled by 50 the recursion is unstable from n = 7 on: there the values are min-sum combinations that grow with every
    layer and iteration, and a 1e-13 change of one exp / log result comes out, on 128 consecutive trials, as 3.5e-6 (n = 7), 3
    (n = 10), 1.7e3 (n = 11) after 4 iterations and as 2e-9, 5e-6, 1e-2 after 2 — linearly in the change. The scaled rows therefore
    have a tolerance of their own, TOL_SCALED, measured the same way over exactly the rows and `iters` it is used on, with the rows
    chosen at MARGIN_SCALED = 100 TOL_SCALED; it covers every code at 1 and 2 iterations and n <= 7 at 4. The ONLY combinations exact
    mode is not compared on are the scaled rows of (10, 512, 8) and (11, 1024, 16) at 4 iterations, where the deviation (0.34 and 62
    even on rows with every leaf above 1e-6) leaves neither the soft nor the hard outputs determined; min-sum mode, which is
    bit-exact, covers them.
"""
import numpy as np

import list_stats_numpy as R
import scl_list_numpy as S

RUN, ERR, UNDET, ITERS_COL = range(4)                        # include/polar_amd.h POLAR_SN_*
MAX_ITERS = 32                                               # POLAR_SCAN_MAX_ITERS
# measure_tol(draws=(0, 1, 2, 3)): 3.1e-9 on the rows MARGIN admits, the largest of four draws of the perturbation (1.6e-9 .. 3.1e-9) —
# the plain rows of (11, 1024, 16) at 4 iterations give it; (10, 512, 8) 1.5e-10, the other codes below 4e-11. TOL is ten times that,
# rounded up to one digit. (Which rows are measured depends on TOL through MARGIN; measure_tol(tol=...) selects them at another
# margin: at 3e-8 the figures are the same.)
TOL = 4e-8
MARGIN = 100 * TOL
# measure_tol(scaled=True, draws=(0, 1, 2, 3)): 0.8e-6 .. 1.8e-6 — (10, 512, 8) at 2 iterations; (7, 64, 8) at 4: 1.9e-7, (11, 1024, 16)
# at 2: 1.4e-7, everything else below 3e-9 — and 3.6e-6 on the 16 rows tests/test_scan.py measures again: this measurement moves
# with the draw, so the largest figure seen counts. Ten times that, rounded up. The values it applies to reach several thousand.
TOL_SCALED = 4e-5
MARGIN_SCALED = 100 * TOL_SCALED


class MarginError(RuntimeError):
    pass


def ms_node(a, b):
    mn = np.minimum(np.abs(a), np.abs(b))
    return np.where(mn == 0, 0.0, np.sign(a) * np.sign(b) * mn)


def perturbed(rng):
    """f_node with every result of its exp / log branch moved by a random relative 1e-13 plus absolute 1e-15."""
    def g(a, b):
        r = S.f_node(a, b)
        small = np.maximum(np.abs(a), np.abs(b)) < 40
        u, w = rng.uniform(-1, 1, r.shape), rng.uniform(-1, 1, r.shape)
        return np.where(small, r * (1 + 1e-13 * u) + 1e-15 * w, r)
    return g


def iterate(code, llr, iters, minsum=False, f=None):
    """`iters` iterations on llr [T, N] -> (leaf [iters, T, N], ext [iters, T, N]): the leaf LLRs in decoding order and the B of layer
    0 after every iteration."""
    llr = np.asarray(llr, np.float64).reshape(-1, code.N)
    T, n, N = len(llr), code.n, code.N
    f = f or (ms_node if minsum else S.f_node)
    keep = {}                                                                 # (layer, node) of a right child -> its B
    leaf = np.zeros((iters, T, N))
    ext = np.zeros((iters, T, N))

    def walk(it, lam, v, a):
        if lam == n:
            leaf[it, :, v] = a[:, 0]
            return np.full((T, 1), np.inf if code.frozen[v] else 0.0)
        a0, a1 = a[:, 0::2], a[:, 1::2]
        b_right = keep.get((lam + 1, 2 * v + 1))
        if b_right is None:
            b_right = np.full((T, 1), np.inf if code.frozen[2 * v + 1] else 0.0) if lam + 1 == n else np.zeros(a0.shape)
        b_left = walk(it, lam + 1, 2 * v, f(a0, a1 + b_right))
        b_right = walk(it, lam + 1, 2 * v + 1, f(a0, b_left) + a1)
        keep[(lam + 1, 2 * v + 1)] = b_right
        b = np.empty(a.shape)
        b[:, 0::2] = f(b_left, b_right + a1)
        b[:, 1::2] = f(b_left, a0) + b_right
        return b

    with np.errstate(invalid="raise", over="raise", divide="raise"):          # (no inf - inf, no overflow: rows are finite)
        for it in range(iters):
            ext[it] = walk(it, 0, 0, llr)
    return leaf, ext


def decode(code, llr, iters, minsum=False, early_stop=False, check=None, f=None, margin=None):
    """SCAN of llr [T, N] -> dict(info [T, K] uint8, info_llr [T, K], ext [T, N], crc_ok, n_iter uint8 [T], leaf, ext_all: every
    iteration's). check (default: exact mode only): MarginError for an unfrozen leaf LLR below `margin` (default MARGIN) at the end
    of any iteration."""
    assert 1 <= iters <= MAX_ITERS and not (early_stop and code.crc == 0)
    leaf, ext = iterate(code, llr, iters, minsum, f)
    T = leaf.shape[1]
    u = (leaf < 0).astype(np.uint8)                                           # (a zero of either sign decides 0)
    ok_it = np.stack([S.crc_ok(code, *S.split(code, u[it])) for it in range(iters)])         # [iters, T]
    n_iter = np.full(T, iters, np.int64)
    if early_stop:
        n_iter = np.where(ok_it.any(axis=0), ok_it.argmax(axis=0) + 1, iters)
    rows = np.arange(T)
    last = leaf[n_iter - 1, rows]
    r = dict(info=u[n_iter - 1, rows][:, code.order[:code.K]], info_llr=last[:, code.order[:code.K]], ext=ext[n_iter - 1, rows],
             crc_ok=ok_it[n_iter - 1, rows].astype(np.uint8), n_iter=n_iter.astype(np.uint8), leaf=leaf, ext_all=ext)
    if check if check is not None else not minsum:
        m, margin = row_margins(code, r), MARGIN if margin is None else margin
        if (m < margin).any():
            raise MarginError("an unfrozen leaf LLR of row %d is %g, below %g" % (int(m.argmin()), float(m.min()), margin))
    return r


LEFT, RIGHT, UP, PAIR = range(4)                             # polar_kernels.h POLAR_SCAN_OP_*
MIXED, FROZEN, UNFROZEN = range(3)                           # POLAR_SCAN_KIND_*


def schedule(code):
    """The kernel's walk (polar_scan.cpp scan_schedule) as (type, lam, v, kl, kr, wb) tuples: nothing walks into an all-frozen
    subtree, an all-unfrozen one has no UP steps, a node of two leaves is one op, the root always gets its B."""
    n = code.n
    unf = np.concatenate([[0], np.cumsum(code.frozen == 0)])

    def kind(l, w):
        c = unf[(w + 1) << (n - l)] - unf[w << (n - l)]
        return FROZEN if c == 0 else UNFROZEN if c == 1 << (n - l) else MIXED
    ops = []

    def go(lam, v):
        kl, kr = kind(lam + 1, 2 * v), kind(lam + 1, 2 * v + 1)
        wb = int(kind(lam, v) == MIXED or lam == 0)
        if lam == n - 1:
            ops.append((PAIR, lam, v, kl, kr, wb))
            return
        if kl != FROZEN:
            ops.append((LEFT, lam + 1, v, kl, kr, 0))
            go(lam + 1, 2 * v)
        if kr != FROZEN:
            ops.append((RIGHT, lam + 1, v, kl, kr, 0))
            go(lam + 1, 2 * v + 1)
        if wb:
            ops.append((UP, lam, v, kl, kr, 1))
    go(0, 0)
    return ops


def pruned(code, llr, iters, minsum=False):
    """iterate() the way the kernel does it: the schedule's ops on the kernel's arrays — one L node per layer, the B of the open left
    child per layer, the B of every right child of layers 1 .. n-1, constants for the B of all-frozen (+inf) and all-unfrozen (0)
    subtrees. Leaves nobody reads (frozen ones) stay 0. -> (leaf [iters, T, N], ext [iters, T, N])"""
    llr = np.asarray(llr, np.float64).reshape(-1, code.N)
    T, n, N, H = len(llr), code.n, code.N, code.N // 2
    f = ms_node if minsum else S.f_node
    off = lambda lam: 2 * N - ((2 * N) >> lam)
    lay, bl, br = np.zeros((T, 2 * N)), np.zeros((T, N)), np.zeros((T, max(n - 1, 0) * H))
    lay[:, :N] = llr
    leaf, ext = np.zeros((iters, T, N)), np.zeros((iters, T, N))
    const = {FROZEN: np.inf, UNFROZEN: 0.0}
    ops = schedule(code)
    for it in range(iters):
        cur = leaf[it - 1].copy() if it else np.zeros((T, N))
        for typ, lam, v, kl, kr, wb in ops:
            if typ in (LEFT, RIGHT):
                m = N >> lam
                par = lay[:, off(lam - 1):off(lam - 1) + 2 * m]
                a0, a1 = par[:, 0::2], par[:, 1::2]
                if typ == LEFT:
                    # (the previous iteration's B: before iteration 1 an internal node's is 0, an all-frozen one's too)
                    b = br[:, (lam - 1) * H + v * m:(lam - 1) * H + (v + 1) * m] if kr == MIXED else const[kr] if it else 0.0
                    lay[:, off(lam):off(lam) + m] = f(a0, a1 + b)
                else:
                    b = bl[:, off(lam) - N:off(lam) - N + m] if kl == MIXED else const[kl]
                    lay[:, off(lam):off(lam) + m] = f(a0, b + np.zeros_like(a0)) + a1
                continue
            m = N >> (lam + 1)
            a = lay[:, off(lam):off(lam) + 2 * m]
            a0, a1 = a[:, 0::2], a[:, 1::2]
            if typ == UP:
                b_l = bl[:, off(lam + 1) - N:off(lam + 1) - N + m] if kl == MIXED else np.full(a0.shape, const[kl])
                b_r = br[:, lam * H + v * m:lam * H + (v + 1) * m] if kr == MIXED else np.full(a0.shape, const[kr])
            else:
                b_l, b_r = np.full(a0.shape, const[kl]), np.full(a0.shape, const[kr])
                if kl != FROZEN:
                    cur[:, 2 * v] = f(a0, a1 + b_r)[:, 0]
                if kr != FROZEN:
                    cur[:, 2 * v + 1] = (f(a0, b_l) + a1)[:, 0]
            if wb:
                b = np.empty((T, 2 * m))
                b[:, 0::2] = f(b_l, b_r + a1)
                b[:, 1::2] = f(b_l, a0) + b_r
                if lam == 0:
                    ext[it] = b
                elif v & 1:
                    br[:, (lam - 1) * H + (v >> 1) * 2 * m:(lam - 1) * H + ((v >> 1) + 1) * 2 * m] = b
                else:
                    bl[:, off(lam) - N:off(lam) - N + 2 * m] = b
        leaf[it] = cur
    return leaf, ext


def row_margins(code, r):
    """[T]: the smallest unfrozen leaf magnitude of any iteration of a decode() result, per row"""
    return np.abs(r["leaf"][:, :, code.order[:code.K + code.crc]]).min(axis=(0, 2))


def forced_coded_bits(code):
    """bool [N]: the coded bits the frozen set alone fixes — where ext is +inf. The encoder's map over "is this bit a known zero":
    x[2j] = xl[j] ^ xr[j] is known iff both are, x[2j + 1] = xr[j] iff xr[j] is."""
    def rec(known):
        if len(known) == 1:
            return known
        h = len(known) // 2
        kl, kr = rec(known[:h]), rec(known[h:])
        x = np.empty(len(known), bool)
        x[0::2] = kl & kr
        x[1::2] = kr
        return x
    return rec(code.frozen.astype(bool))


def counters(r, sent, crc):
    """The POLAR_SN_N counters of polar_mc_batch_scan for a decode() result against the sent words."""
    err = (r["info"] != sent).any(axis=1)
    return np.array([len(sent), err.sum(), (err & (r["crc_ok"] == 1)).sum() if crc else 0, r["n_iter"].astype(np.int64).sum()], np.uint64)


def same_soft(got, want, tol):
    """finite where `want` is, within tol there, and the same +inf pattern"""
    fin = np.isfinite(want)
    return bool((np.isposinf(got) == ~fin).all() and (np.isfinite(got) == fin).all() and
                (np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0)) <= tol).all())


# ---- the inputs the CPU and the GPU tests share -----------------------------------------------------------------------------------
# the codes of tests/test_gpu_scan.py, (n, K, crc): the root is the leaf pair; one quad; N below a wave; one wave; lanes loop twice at
# layer 0; a mid-size code; the LDS maximum. REFUSED is above the kernel's cap.
CODES = [(1, 1, 0), (2, 2, 0), (5, 16, 8), (6, 32, 8), (7, 64, 8), (10, 512, 8), (11, 1024, 16)]
REFUSED = (12, 2048, 16)
ROWS, SEED, EBNO, SCALE = 64, 1, 1.5, 50.0
ITERS = (1, 2, 4)


def scaled_iters(key):
    """the `iters` at which exact mode is compared on rows scaled by SCALE: all of ITERS up to n = 7, 1 and 2 at n = 10 and 11 — the
    two combinations left out, (10, 512, 8) and (11, 1024, 16) at 4 iterations, are the ones no tolerance covers (module docstring)"""
    return ITERS if key[0] <= 7 else (1, 2)


# (n, K, crc), iters -> (ERR, UNDET, sum of n_iter with early stop, ERR with early stop, UNDET with early stop) over trials 0 .. 255 of
# seed 1 at Eb/N0 1.5 dB (list_stats_numpy.stats_inputs), exact arithmetic. tests/test_scan.py recomputes all of it. (One iteration
# of SCAN is weaker than SC — 153 and 114 of these rows fail there, flip_numpy.TABLE —: a right child sees a soft 0 where SC hands it
# a decision.) These trials are taken as they come: 11 of the first code's rows and 18 of the second's have a leaf below MARGIN, the
# smallest 1e-8 and 7e-11, against a measured deviation of 2e-12 and 3e-11 on those rows.
TABLE = [
    ((6, 32, 8), 1, 185, 1, 256, 185, 1),
    ((6, 32, 8), 2, 172, 1, 445, 170, 2),
    ((6, 32, 8), 4, 169, 1, 782, 165, 3),
    ((7, 64, 8), 1, 161, 0, 256, 161, 0),
    ((7, 64, 8), 2, 148, 2, 417, 141, 2),
    ((7, 64, 8), 4, 139, 1, 688, 128, 3),
]
# early stop at (6, 32, 8), 4 iterations, on the TABLE rows: how many rows stop after iteration 1, 2, 3, 4 (index = n_iter), and how many
# of the last never pass
EARLY_HIST = [0, 67, 19, 3, 167]
EARLY_NEVER = 166
# launch geometry at (5, 16, 8): batches (rows of seed EDGE_SEED + B), and one row more than the kernel's launch has blocks (8192)
EDGE_B = [1, 63, 65, 257]
EDGE_SEED = 30
GRID_CAP_ROWS = 8193

_cache = {}


def code_of(key):
    """(oracle, Code) of (n, K, crc), once per process."""
    if key not in _cache:
        o = R.oracle(*key)
        _cache[key] = (o, S.Code(o))
    return _cache[key]


def clean_rows(key, rows=ROWS, seed=SEED, ebno=EBNO, scale=1.0, margin=None, iters=None):
    """(llr [rows, N] times scale, sent [rows, K], trial numbers) — the first `rows` trials of `seed` at `ebno` on which the exact
    model has no unfrozen leaf below `margin` in any of `iters` iterations; once per process. Defaults: plain rows MARGIN and
    max(ITERS), scaled rows MARGIN_SCALED and max(scaled_iters(key))."""
    margin = margin if margin is not None else MARGIN if scale == 1.0 else MARGIN_SCALED
    iters = iters or (max(ITERS) if scale == 1.0 else max(scaled_iters(key)))
    k = ("clean", key, rows, seed, ebno, scale, margin, iters)
    if k not in _cache:
        o, code = code_of(key)
        got, t0 = [], 0
        while sum(len(g[2]) for g in got) < rows:
            step = max(64, rows // 2)
            llr, sent = o.synth_llr(seed, t0, step, o.snr_sqrt_linear(ebno))
            good = row_margins(code, decode(code, scale * llr, iters, check=False)) >= margin
            got.append((scale * llr[good], sent[good], t0 + np.flatnonzero(good)))
            t0 += step
        _cache[k] = tuple(np.concatenate([g[i] for g in got])[:rows] for i in range(3))
    return _cache[k]


def plain_rows(key, rows=ROWS, seed=SEED, ebno=EBNO):
    """(llr [rows, N], sent [rows, K]): the first `rows` trials as they come — what min-sum mode, bit-exact on any row, is compared on"""
    o, _ = code_of(key)
    return o.synth_llr(seed, 0, rows, o.snr_sqrt_linear(ebno))


class TailTables:
    """An explicit code (n = 4, K = 5, no CRC) whose frozen set fixes coded bits — the last leaves frozen, a right child all frozen
    beside a left one that is not: what no construction produces and the kernel's pruning must still get right."""
    n, K, crc = 4, 5, 0

    def frozen(self):
        return [1, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0, 1, 1, 1, 1, 1]

    def order(self):
        return [3, 5, 6, 9, 10, 0, 1, 2, 4, 7, 8, 11, 12, 13, 14, 15]

    def crc_matrix(self):
        return []


def tail_rows(rows=32):
    return np.random.default_rng(5).normal(1.0, 2.0, (rows, 16))


def special_rows(key):
    """the all-zero row and a row of one large value, [2, N]"""
    N = 1 << key[0]
    x = np.zeros((2, N))
    x[1, N // 3] = -1e6
    return x


def table_reference(key, iters, early_stop=False):
    """(code, llr, sent, decode() result) of the sweep's 256 rows, once per process."""
    k = ("table", key, iters, early_stop)
    if k not in _cache:
        o, code = code_of(key)
        llr, sent = R.stats_inputs(o)
        _cache[k] = (code, llr, sent, decode(code, llr, iters, early_stop=early_stop, check=False))
    return _cache[k]


def exact_test_rows(rows=ROWS, table_rows=256, edge=True, scaled=False, tol=None):
    """Every (key, llr, iters) the exact-mode tests compare soft values on under TOL (scaled=False: per code the clean rows at
    max(ITERS); the sweep's rows; the rows of the launch geometry) or under TOL_SCALED (scaled=True: per code the clean rows times
    SCALE at every one of scaled_iters). tol: select the rows at the margin 100 tol instead of the module's."""
    m = None if tol is None else 100 * tol
    for key in CODES:
        if scaled:
            for it in scaled_iters(key):
                yield key, clean_rows(key, rows, scale=SCALE, margin=m)[0], it
        else:
            yield key, clean_rows(key, rows, margin=m)[0], max(ITERS)
    if scaled:
        return
    for key in ((6, 32, 8), (7, 64, 8)):
        o, _ = code_of(key)
        yield key, R.stats_inputs(o)[0][:table_rows], max(ITERS)
    if edge:
        for B in EDGE_B + [GRID_CAP_ROWS]:
            yield (5, 16, 8), clean_rows((5, 16, 8), B, seed=EDGE_SEED + B, margin=m)[0], max(ITERS)


def measure_tol(rows=ROWS, table_rows=256, edge=True, draws=(0,), scaled=False, tol=None):
    """(the largest absolute deviation of any finite info_llr / ext entry between the model and the model with perturbed f over
    exact_test_rows and over the perturbations drawn from the seeds `draws`, the same per (code, iters)). TOL (scaled: TOL_SCALED)
    is ten times the former."""
    worst = {}
    cases = [(key, llr, iters, seed) for seed in draws for key, llr, iters in exact_test_rows(rows, table_rows, edge, scaled, tol)]
    rngs = {seed: np.random.default_rng(seed) for seed in draws}
    for key, llr, iters, seed in cases:
        _, code = code_of(key)
        a = decode(code, llr, iters, check=False)
        b = decode(code, llr, iters, check=False, f=perturbed(rngs[seed]))
        d = 0.0
        for name in ("info_llr", "ext"):
            fin = np.isfinite(a[name])
            assert (np.isfinite(b[name]) == fin).all() and not np.isnan(a[name]).any() and not np.isnan(b[name]).any()
            if fin.any():
                d = max(d, float(np.abs(a[name][fin] - b[name][fin]).max()))
        worst[(key, iters)] = max(worst.get((key, iters), 0.0), d)
    return max(worst.values()), worst
