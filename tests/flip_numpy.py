"""SC-Flip (include/polar_amd.h polar_decode_sc_flip_batch) restated in numpy on the node arithmetic of
tests/scl_list_numpy.py: what the device is tested against, and the inputs and expected counts the CPU and the GPU tests share.

A pass is plain successive cancellation in the LLR domain: leaf phi (decoding order) decides 0 if frozen, else 1 iff its LLR is
negative; at the flip position that decision is inverted. Pass 0 flips nothing. Its unfrozen leaves, ordered by |LLR| ascending and
by position where magnitudes are equal (a stable sort), give the candidates; retry t is a whole pass with candidate t flipped; the
first word whose decided check bits are those the CRC matrix gives for its info bits is delivered.

numpy's exp / log and the kernel's table-driven ones agree to about 1e-13 relative. A row whose result could depend on that — two of
the first T_eff + 1 magnitudes closer than 1e-9 relative, or an unfrozen leaf LLR below 1e-9 in magnitude, whose sign decides a bit —
raises MarginError instead of being decoded.
"""
import os

import numpy as np

import list_stats_numpy as R
import scl_list_numpy as S

RUN, ERR, UNDET, FIRST, FLIPPED, DECODES = range(6)          # include/polar_amd.h POLAR_FL_*
FLIP_MAX = 64                                                # POLAR_FLIP_MAX
MARGIN = 1e-9


class MarginError(RuntimeError):
    pass


def sc_pass(code, llr, flip=None):
    """One SC pass over llr [T, N] with the flip positions flip [T] (-1 or None: none) -> (u [T, N] uint8, leaf [T, N]): the
    decisions and the leaf LLRs, both in decoding order."""
    llr = np.asarray(llr, np.float64).reshape(-1, code.N)
    T = len(llr)
    flip = np.full(T, -1, np.int64) if flip is None else np.asarray(flip, np.int64)
    u = np.zeros((T, code.N), np.uint8)
    leaf = np.zeros((T, code.N))

    def rec(a, phi0):
        size = a.shape[1]
        if size == 1:
            leaf[:, phi0] = a[:, 0]
            bit = np.zeros(T, np.uint8) if code.frozen[phi0] else ((a[:, 0] < 0) ^ (flip == phi0)).astype(np.uint8)
            u[:, phi0] = bit
            return bit[:, None]
        xl = rec(S.f_node(a[:, 0::2], a[:, 1::2]), phi0)
        xr = rec(S.g_node(a[:, 0::2], a[:, 1::2], xl), phi0 + size // 2)
        x = np.empty((T, size), np.uint8)
        x[:, 0::2] = xl ^ xr
        x[:, 1::2] = xr
        return x

    rec(llr, 0)
    return u, leaf


def t_eff(code, T):
    return min(int(T), code.K + code.crc)


def candidates(code, leaf, T, check=True):
    """(cand [rows, T] int32, mag [rows, T]) of pass 0's leaf LLRs: the T_eff unfrozen positions of smallest magnitude, ascending,
    equal magnitudes by position; entries from T_eff on are -1 / +inf."""
    rows, te = len(leaf), t_eff(code, T)
    unfrozen = np.flatnonzero(code.frozen == 0)
    m = np.abs(leaf[:, unfrozen])
    idx = np.argsort(m, axis=1, kind="stable")
    ms = np.take_along_axis(m, idx, axis=1)
    if check:
        if (m < MARGIN).any():
            raise MarginError("an unfrozen leaf LLR of row %d is below %g" % (int(np.argwhere(m < MARGIN)[0][0]), MARGIN))
        head = ms[:, :te + 1]
        gap = np.diff(head, axis=1) / np.maximum(head[:, 1:], 1e-300)
        if gap.size and (gap < MARGIN).any():
            raise MarginError("two of the first %d magnitudes of row %d are closer than %g relative" %
                              (te + 1, int(np.argwhere(gap < MARGIN)[0][0]), MARGIN))
    cand = np.full((rows, T), -1, np.int32)
    mag = np.full((rows, T), np.inf)
    cand[:, :te] = unfrozen[idx[:, :te]]
    mag[:, :te] = ms[:, :te]
    return cand, mag


def min_margins(code, leaf, T):
    """(smallest relative gap among the first T_eff + 1 sorted magnitudes, smallest unfrozen magnitude) over all rows."""
    te = t_eff(code, T)
    m = np.sort(np.abs(leaf[:, code.frozen == 0]), axis=1)
    head = m[:, :te + 1]
    gap = np.diff(head, axis=1) / np.maximum(head[:, 1:], 1e-300)
    return (float(gap.min()) if gap.size else np.inf), float(m.min())


def decode(code, llr, T, check=True):
    """SC-Flip of llr [rows, N] with at most T retries -> dict(info [rows, K] uint8, crc_ok, n_dec uint8 [rows], flip int32 [rows],
    cand int32 [rows, T], mag [rows, T], u0 [rows, N] pass 0's decisions, leaf0 [rows, N] pass 0's leaf LLRs). Retries check their
    own unfrozen leaf LLRs against MARGIN as well."""
    assert code.crc > 0 and 0 <= T <= FLIP_MAX
    llr = np.asarray(llr, np.float64).reshape(-1, code.N)
    rows, te = len(llr), t_eff(code, T)
    u0, leaf0 = sc_pass(code, llr)
    cand, mag = candidates(code, leaf0, T, check)
    info, chk = S.split(code, u0)
    info = info.copy()
    ok = S.crc_ok(code, info, chk)
    n_dec = np.where(ok, 1, te + 1).astype(np.uint8)
    flip = np.full(rows, -1, np.int32)
    left = np.flatnonzero(~ok)
    for t in range(te):
        if not len(left):
            break
        u, leaf = sc_pass(code, llr[left], cand[left, t])
        if check and (np.abs(leaf[:, code.frozen == 0]) < MARGIN).any():
            raise MarginError("an unfrozen leaf LLR of retry %d is below %g" % (t, MARGIN))
        i_t, c_t = S.split(code, u)
        good = S.crc_ok(code, i_t, c_t)
        hit = left[good]
        info[hit], n_dec[hit], flip[hit] = i_t[good], t + 2, cand[hit, t]
        ok[hit] = True
        left = left[~good]
    return dict(info=info, crc_ok=ok.astype(np.uint8), n_dec=n_dec, flip=flip, cand=cand, mag=mag, u0=u0, leaf0=leaf0)


def counters(r, sent):
    """The POLAR_FL_N counters of polar_mc_batch_flip for a decode() result against the sent words."""
    err = (r["info"] != sent).any(axis=1)
    ok = r["crc_ok"] == 1
    return np.array([len(sent), err.sum(), (err & ok).sum(), (ok & (r["n_dec"] == 1)).sum(), (ok & (r["n_dec"] > 1)).sum(),
                     r["n_dec"].astype(np.int64).sum()], np.uint64)


def shares(r):
    """[first-pass rows, rows a retry delivered, failed rows]."""
    ok = r["crc_ok"] == 1
    return [int((ok & (r["n_dec"] == 1)).sum()), int((ok & (r["n_dec"] > 1)).sum()), int((~ok).sum())]


# ---- the inputs the CPU and the GPU tests share -----------------------------------------------------------------------------------
# (n, K, crc), T -> ([FIRST, FLIPPED, failed], ERR, UNDET, DECODES) over trials 0 .. 255 of seed 1 at Eb/N0 1.5 dB
# (list_stats_numpy.stats_inputs). tests/test_flip.py recomputes all of it, and that no row raises MarginError.
TABLE = [
    ((6, 32, 8), 4, [103, 60, 93], 95, 2, 729),
    ((6, 32, 8), 8, [103, 69, 84], 88, 4, 1089),
    ((7, 64, 8), 8, [142, 62, 52], 56, 4, 867),
    ((7, 64, 8), 16, [142, 68, 46], 50, 4, 1252),
]
# histograms of n_dec (index = n_dec, 0 .. T + 1) of the rows above
TABLE_HIST = {
    ((6, 32, 8), 4): [0, 103, 37, 9, 10, 97],
    ((6, 32, 8), 8): [0, 103, 37, 9, 10, 4, 1, 4, 1, 87],
    ((7, 64, 8), 8): [0, 142, 16, 17, 8, 5, 5, 3, 6, 54],
    ((7, 64, 8), 16): [0, 142, 16, 17, 8, 5, 5, 3, 6, 2, 1, 1, 2, 2, 0, 0, 0, 46],
}
# larger rows, stored in tests/golden/flip_fixtures.npz by tests/golden/make_flip_fixtures.py:
# rows, (n, K, crc), T, seed, Eb/N0 -> [FIRST, FLIPPED, failed]
FIXTURES = [
    (64, (5, 16, 8), 64, 1, 1.5, [16, 25, 23]),
    (48, (10, 512, 8), 8, 1, 1.5, [26, 9, 13]),
    (32, (11, 1024, 16), 8, 1, 1.5, [20, 6, 6]),
    (32, (11, 1024, 16), 8, 1, 2.0, [30, 2, 0]),
    (12, (12, 2048, 16), 4, 1, 1.5, [9, 0, 3]),
]
# the grid edges of tests/test_gpu_flip.py at (6, 32, 8), T = EDGE_T: B rows of seed edge_seed(B, Eb/N0), and one batch of one row more
# than the kernel's launch has blocks (8192) — B, seed, Eb/N0, T. At -10 dB the model refuses many rows (leaf LLRs below 1e-9) and an
# 8-bit CRC accepts one wrong word in 256 by chance: the seeds of that point were searched on the CPU (from 100 upwards, the first
# hit) for rows on which the model raises no MarginError and accepts nothing, so that "every retry is spent, nothing is delivered"
# can be asserted as such. tests/test_flip.py recomputes it. The rows scaled by MIN_SUM_SCALE take the min-sum branch of the f-node.
EDGE_B, EDGE_SEED, EDGE_EBNO, EDGE_T = [1, 63, 65, 257], 30, (8.0, -10.0, 1.5), 4
EDGE_SEED_M10 = {1: 100, 63: 102, 65: 102, 257: 453}


def edge_seed(B, ebno):
    return EDGE_SEED_M10[B] if ebno == -10.0 else EDGE_SEED + B


GRID_CAP_CASE = (8193, 5, 1.5, 2)
MIN_SUM_SCALE, MIN_SUM_ROWS = 50.0, 64
FIXTURE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flip_fixtures.npz")

_cache = {}


def reference(key, T):
    """(oracle, code, llr, sent, decode() result) of the shared inputs of code `key` = (n, K, crc) with T retries, once per process."""
    if key not in _cache:
        o = R.oracle(*key)
        _cache[key] = (o, S.Code(o)) + tuple(R.stats_inputs(o))
    if (key, T) not in _cache:
        o, code, llr, sent = _cache[key]
        _cache[(key, T)] = decode(code, llr, T)
    return _cache[key] + (_cache[(key, T)],)


def fixture_inputs(i):
    """(oracle, code, llr, sent) of row i of FIXTURES, from the oracle's channel."""
    rows, key, T, seed, ebno, _ = FIXTURES[i]
    o = R.oracle(*key)
    llr, sent = o.synth_llr(seed, 0, rows, o.snr_sqrt_linear(ebno))
    return o, S.Code(o), llr, sent


def load_fixtures():
    """The stored results: a list of dicts (llr_sha, sent, info, crc_ok, n_dec, flip, cand, mag) in the order of FIXTURES. The rows
    themselves are not stored (fixture_inputs regenerates them); llr_sha is the sha256 of their bytes, as uint8 [32]."""
    z = np.load(FIXTURE_FILE)
    return [{k: z["%d_%s" % (i, k)] for k in ("llr_sha", "sent", "info", "crc_ok", "n_dec", "flip", "cand", "mag")}
            for i in range(len(FIXTURES))]


def llr_sha(llr):
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(llr, np.float64).tobytes()).digest(), np.uint8)
