"""A plain numpy successive-cancellation LIST decoder that returns every survivor — the independent statement the list output
of the device decoder (decode_scl_llr_list) is tested against — and the pieces the tests need beside it.

Arithmetic: the reference's (PolarCode.cpp:437-451, 483, 505-506) — the f-node takes the min-sum branch when max(|a|, |b|) is
not below 40 and log((exp(a+b)+1)/(exp(a)+exp(b))) otherwise, the g-node is (1 - 2u) a + b, a leaf adds log(1 + exp(-llr)) for
a decision 0 and log(1 + exp(llr)) for a decision 1 (+inf where the argument of exp is above 709.78). numpy's exp / log are not
glibc's to the last bit: metrics agree with the oracle's to about 1e-13 relative, the tests allow 1e-10.

The list search (scl_list, N <= 128) keeps the L smallest of the 2 L fork metrics at every unfrozen leaf. It does NOT restate the
reference's tie rule: where the L-th and the (L+1)-th metric are equal, or two survivors end with equal metrics, the set or the
order would depend on that rule, and the function raises TieError instead. The forced pass (forced_path_metric) has no such
limit and is vectorised over paths: it works at N = 2048.
"""
import numpy as np


class TieError(RuntimeError):
    pass


class Code:
    """The tables of a code, taken from an object that has n, K, crc, frozen(), order(), crc_matrix() (tests/oracle_lib.py)."""

    def __init__(self, src):
        self.n, self.N, self.K, self.crc = src.n, 1 << src.n, src.K, src.crc
        self.frozen = np.asarray(src.frozen(), np.uint8).copy()
        self.order = np.asarray(src.order(), np.int64).copy()
        self.crcm = np.asarray(src.crc_matrix(), np.uint8).reshape(max(self.crc, 0), self.K).copy()


def crc_bits(code, info):
    """The crc check bits the CRC matrix gives for info [..., K] (PolarCode.cpp:78-85)."""
    info = np.asarray(info, np.int64)
    return ((info @ code.crcm.T.astype(np.int64)) % 2).astype(np.uint8)


def crc_ok(code, info, check=None):
    """crc_check (PolarCode.cpp:93-108) from the CRC matrix: do the decided check bits `check` [..., crc] equal the parity of
    info [..., K]? crc == 0: True."""
    info = np.asarray(info)
    if code.crc == 0:
        return np.ones(info.shape[:-1], bool)
    return (crc_bits(code, info) == np.asarray(check, np.uint8)).all(axis=-1)


def word(code, info, check=None):
    """The decision vector u [..., N] (decoding order) of info [..., K] and check bits [..., crc] (None: the CRC matrix's)."""
    info = np.asarray(info, np.uint8)
    u = np.zeros(info.shape[:-1] + (code.N,), np.uint8)
    u[..., code.order[:code.K]] = info
    if code.crc:
        u[..., code.order[code.K:code.K + code.crc]] = crc_bits(code, info) if check is None else check
    return u


def split(code, u):
    """(info [..., K], check [..., crc]) of decision vectors u [..., N]."""
    u = np.asarray(u)
    return u[..., code.order[:code.K]], u[..., code.order[code.K:code.K + code.crc]]


def f_node(a, b):
    fa, fb = np.abs(a), np.abs(b)
    small = np.maximum(fa, fb) < 40
    a_, b_ = np.where(small, a, 0.0), np.where(small, b, 0.0)
    exact = np.log((np.exp(a_ + b_) + 1) / (np.exp(a_) + np.exp(b_)))
    return np.where(small, exact, np.sign(a) * np.sign(b) * np.minimum(fa, fb))


def g_node(a, b, u):
    return (1 - 2 * u.astype(np.float64)) * a + b


def leaf_cost(x):
    """log(1 + exp(x)), +inf where x is above 709.78 (glibc's exp overflows there)."""
    x = np.asarray(x, np.float64)
    big = x > 709.78
    return np.where(big, np.inf, np.log(1 + np.exp(np.where(big, 0.0, x))))


def forced_path_metric(code, llr, u):
    """SC along given decision vectors: llr [N], u [N] or [R, N] (decoding order, frozen positions included) -> the metric of
    each path, summed in leaf order."""
    u = np.asarray(u, np.uint8)
    single = u.ndim == 1
    u2 = u.reshape(-1, code.N)
    pm = np.zeros(u2.shape[0])

    def rec(a, ub):
        nonlocal pm
        S = a.shape[1]
        if S == 1:
            pm = pm + leaf_cost(np.where(ub[:, 0] == 0, -a[:, 0], a[:, 0]))
            return ub
        xl = rec(f_node(a[:, 0::2], a[:, 1::2]), ub[:, :S // 2])
        xr = rec(g_node(a[:, 0::2], a[:, 1::2], xl), ub[:, S // 2:])
        x = np.empty((a.shape[0], S), np.uint8)
        x[:, 0::2] = xl ^ xr
        x[:, 1::2] = xr
        return x

    rec(np.broadcast_to(np.asarray(llr, np.float64), (u2.shape[0], code.N)), u2)
    return pm[0] if single else pm


def scl_list(code, llr, L):
    """Every survivor of a list-of-L decode of llr [N]: a list of dicts (u [N], info [K], pm, crc_ok) in the order CRC pass
    first, then metric ascending. Raises TieError where the result would depend on the reference's tie rule."""
    n, N = code.n, code.N
    assert N <= 128, "the list search is for small codes; forced_path_metric has no such limit"
    A = [np.asarray(llr, np.float64).reshape(1, N)] + [np.zeros((1, N >> lam)) for lam in range(1, n + 1)]
    CL = [np.zeros((1, N >> lam), np.uint8) for lam in range(n + 1)]
    CR = [np.zeros((1, N >> lam), np.uint8) for lam in range(n + 1)]
    U = np.zeros((1, N), np.uint8)
    pm = np.zeros(1)
    for phi in range(N):
        lam_top = 1 if phi == 0 else n - ((phi & -phi).bit_length() - 1)
        for lam in range(lam_top, n + 1):
            a, b = A[lam - 1][:, 0::2], A[lam - 1][:, 1::2]
            A[lam] = g_node(a, b, CL[lam]) if (phi >> (n - lam)) & 1 else f_node(a, b)
        v = A[n][:, 0]
        if code.frozen[phi]:
            pm = pm + leaf_cost(-v)
            bit = np.zeros(len(pm), np.uint8)
        else:
            na = len(pm)
            m = np.concatenate([pm + leaf_cost(-v), pm + leaf_cost(v)])       # decision 0 of every path, then decision 1
            keep = np.argsort(m, kind="stable")
            if 2 * na > L:
                if m[keep[L - 1]] == m[keep[L]]:
                    raise TieError("fork metrics %d and %d are equal at leaf %d" % (L, L + 1, phi))
                keep = np.sort(keep[:L])
            src, bit = keep % na, (keep // na).astype(np.uint8)
            A = [x[src] if x.shape[0] == na else x for x in A]
            CL, CR, U, pm = [x[src] for x in CL], [x[src] for x in CR], U[src], m[keep]
        U[:, phi] = bit
        if phi & 1:
            CR[n][:, 0] = bit
            lam, ph = n, phi                                              # recursivelyUpdateC (PolarCode.cpp:457-473)
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
    rows = [dict(u=U[i], info=info[i], pm=float(pm[i]), crc_ok=bool(ok[i])) for i in range(len(pm))]
    rows.sort(key=lambda r: (not r["crc_ok"], r["pm"]))
    return rows


def best(rows):
    """findMostProbablePath (PolarCode.cpp:609-644) on scl_list's rows: the smallest metric among the paths that pass the CRC, among
    all if none does. (Ties were excluded by scl_list; rows whose every metric is +inf are not restated here.)"""
    passing = [r for r in rows if r["crc_ok"]] or rows
    return min(passing, key=lambda r: r["pm"])


# ---- the inputs the CPU and the GPU tests of the list output share -----------------------------------------------------------
LIST_CASES = [(5, 16, 0, 4), (6, 32, 8, 8), (7, 64, 8, 4)]     # (n, K, crc, L)
LIST_ROWS = 64
LIST_EBNO = 1.5
# chosen on the CPU so that scl_list raises TieError in none of the 192 rows (nor at L = 1, 3, 6 on the first code): a condition on
# the inputs, checked by tests/test_scl_list.py
LIST_SEED = 1


def list_inputs(o):
    """The 64 rows of an oracle object's code: (llr [64, N], sent info [64, K])."""
    return o.synth_llr(LIST_SEED, 0, LIST_ROWS, o.snr_sqrt_linear(LIST_EBNO))
