"""Symbol rows shared by the MLC tests (test_mlc.py, test_gpu_mlc.py, test_gpu_lane_rounds.py): the ordinary rows of
mlc_numpy.synth with the degenerate rows written among them, in the manner of p1_rows. The MLC receiver is the arithmetic of the
probability-domain decoders behind a demapper, so its degenerate inputs are symbols: one whose exponentials all underflow (0 / 0 in
the demapper), a NaN, an infinity, symbols that sit exactly between two points, and symbols so clean that exact 0.0 / 1.0
probabilities enter the decoder. Every comparison built on them is equality of doubles (p1_rows.rows_that_differ)."""
import numpy as np

import mlc_numpy as R

EDGE_KINDS = ("far", "nan", "inf", "mid", "all_far", "loud", "clean")


def bec_code(N, K, eps=0.32):
    """(frozen, order) of the length-N polar code for an erasure channel (the K positions of the smallest Bhattacharyya
    parameters, natural order), with the info order shuffled: a code that decodes, for the sizes where that matters."""
    z = np.array([eps])
    while z.size < N:
        z = np.stack([2 * z - z * z, z * z], axis=1).reshape(-1)
    best = np.argsort(z, kind="stable")
    rng = np.random.default_rng(N + K)
    order = np.concatenate([rng.permutation(best[:K]), best[K:]]).astype(np.uint16)
    frozen = np.ones(N, np.uint8)
    frozen[order[:K]] = 0
    return frozen, order


def edge_row(kind, y_row, clean_row):
    """The degenerate row `kind`, made from the ordinary row y_row and its noiseless symbols clean_row."""
    y = np.array(y_row, np.float64)
    if kind == "far":                   # one symbol whose exponentials all underflow: p1 = 0 / 0 at one position of every level
        y[y.shape[0] // 2] = 1e3
    elif kind == "nan":                 # one NaN symbol
        y[0] = np.nan
    elif kind == "inf":                 # the last symbol -inf: |d|^2 = inf, every exponential exactly 0
        y[-1] = -np.inf
    elif kind == "mid":                 # every symbol exactly 0.0: the two innermost points tie
        y[:] = 0.0
    elif kind == "all_far":             # 0 / 0 at every position
        y[:] = 1e3
    elif kind == "loud":                # the whole row x 6: exact 0.0 / 1.0 in the level-0 probabilities
        y *= 6.0
    elif kind == "clean":               # the noiseless symbols
        y[:] = clean_row
    else:
        raise ValueError(kind)
    return y


def where(B, every=0):
    """[(row, kind index)]: the degenerate rows overwrite the first rows (as many as B holds); with every > 0 also the rows every,
    2 * every, ... in turn (p1_rows.rows)."""
    w = [(k, k) for k in range(min(B, len(EDGE_KINDS)))]
    if every:
        w += [(r, (r // every - 1) % len(EDGE_KINDS)) for r in range(every, B, every)]
    return w


def rows(frozen, order, K, cid, seed, trial0, B, snr_db, every=0):
    """B symbol rows [B][M] at snr_db with the degenerate rows of where(B, every) written over the ordinary ones, and the sent info
    [B][K]. The result is read-only."""
    trials = np.arange(trial0, trial0 + B, dtype=np.uint64)
    y, info = R.synth(frozen, order, K, cid, seed, trials, snr_db)
    x = R.modulate(R.encode(frozen, order, K, info, cid)[0], cid)
    for r, k in where(B, every):
        y[r] = edge_row(EDGE_KINDS[k], y[r], x[r])
    y.setflags(write=False)
    info.setflags(write=False)
    return y, info
