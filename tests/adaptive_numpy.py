"""The adaptive list decoder (include/polar_amd.h polar_decode_scl_llr_adaptive_batch) restated with the numpy list decoder of
tests/scl_list_numpy.py: what the device is tested against, and the inputs and expected counts the CPU and the GPU tests share."""
import numpy as np

import list_stats_numpy as R
import scl_list_numpy as S

RUN, ERR, UNDET, STAGE0 = 0, 1, 2, 3          # include/polar_amd.h POLAR_AD_*

# (n, K, crc), schedule -> (codewords delivered by each stage, block errors, accepted words) over trials 0 .. 255 of seed 1 at
# Eb/N0 1.5 dB (list_stats_numpy.stats_inputs). Computed on a CPU with this file; scl_list raises TieError at no stage of any of
# them and every stage is non-empty (tests/test_adaptive.py recomputes all of it: no GPU test can skip a row).
TABLE = [
    ((6, 32, 8), (1, 2, 4, 8), [103, 40, 30, 83], 63, 196),
    ((6, 32, 8), (3, 6), [161, 95], 71, 186),
    ((7, 64, 8), (1, 2, 8), [142, 41, 73], 30, 227),
    ((7, 64, 8), (1, 4, 32), [142, 68, 46], 22, 242),
]
# single-stage schedules decoded on every row (tie-free on all 256: they are list_stats_numpy.STATS_CASES)
SINGLE = [((6, 32, 8), 8), ((7, 64, 8), 4)]

_lists = {}


def survivors(code, key, i, llr_row, L):
    """scl_list of row i of the shared inputs of code `key`, computed once per (code, row, list size)."""
    k = (key, i, L)
    if k not in _lists:
        _lists[k] = S.scl_list(code, llr_row, L)
    return _lists[k]


def adaptive(code, llr, Ls, key=None):
    """(info [T, K] uint8, pm [T], stage [T] uint8, crc_ok [T] uint8) of llr [T, N] under the schedule Ls: the first stage whose
    winner (scl_list + best) passes the CRC delivers, the last one in any case. TieError (scl_list) is not caught. `key`: the rows
    are the shared inputs of that code — their lists are kept for the other schedules."""
    llr = np.asarray(llr, np.float64).reshape(-1, code.N)
    T = len(llr)
    info = np.zeros((T, code.K), np.uint8)
    pm = np.zeros(T)
    stage = np.zeros(T, np.uint8)
    ok = np.zeros(T, np.uint8)
    for i in range(T):
        for s, L in enumerate(Ls):
            rows = survivors(code, key, i, llr[i], L) if key is not None else S.scl_list(code, llr[i], L)
            w = S.best(rows)
            if w["crc_ok"] or s == len(Ls) - 1:
                info[i], pm[i], stage[i], ok[i] = w["info"], w["pm"], s, 1 if w["crc_ok"] else 0
                break
    return info, pm, stage, ok


def counters(info, stage, ok, sent, n_s):
    """The 3 + n_s counters of polar_mc_batch_adaptive for delivered words against the sent ones."""
    err = (info != sent).any(axis=1)
    c = [len(info), int(err.sum()), int((err & (ok == 1)).sum())] + [int((stage == s).sum()) for s in range(n_s)]
    return np.array(c, np.uint64)


_cache = {}


def reference(key, Ls):
    """(oracle, code, llr, sent, (info, pm, stage, crc_ok)) of the shared inputs of code `key` = (n, K, crc) under the schedule Ls,
    computed once per process."""
    Ls = tuple(Ls)
    if key not in _cache:
        o = R.oracle(*key)
        _cache[key] = (o, S.Code(o)) + tuple(R.stats_inputs(o))
    if (key, Ls) not in _cache:
        o, code, llr, sent = _cache[key]
        _cache[(key, Ls)] = adaptive(code, llr, Ls, key)
    return _cache[key] + (_cache[(key, Ls)],)
