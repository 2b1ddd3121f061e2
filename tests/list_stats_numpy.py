"""The five counters of the list statistics (include/polar_amd.h POLAR_LS_*) restated with the numpy list decoder of
tests/scl_list_numpy.py: what polar_mc_batch_list is tested against, and the inputs the CPU and the GPU tests share."""
import numpy as np

import scl_list_numpy as S

RUN, ERR, MISS, UNDET, ML = range(5)

# (n, K, crc, L): trials 0 .. 255 of seed 1 at Eb/N0 1.5 dB. Chosen on the CPU so that scl_list raises TieError in none of them and the
# winner's metric is nowhere near the sent word's (tests/test_list_stats.py checks both: no GPU test can skip a row)
STATS_CASES = [(5, 16, 0, 4), (6, 32, 8, 8), (7, 64, 8, 4), (5, 16, 0, 1)]
STATS_T = 256
STATS_SEED = 1
STATS_EBNO = 1.5


def oracle(n, K, crc):
    from oracle_lib import Oracle
    return Oracle(n, K, 0.32, crc, srand=1)


def stats_inputs(o):
    """(llr [256, N], sent info [256, K]) of an oracle object's code."""
    return o.synth_llr(STATS_SEED, 0, STATS_T, o.snr_sqrt_linear(STATS_EBNO))


def classify(code, llr, sent, L):
    """(counters [5], smallest relative gap |pm_winner - pm_sent| / max(1, |pm_sent|) over the error rows) of a list-of-L decode
    of llr [T, N] against the sent info [T, K]. TieError (scl_list) is not caught."""
    c = np.zeros(5, np.uint64)
    gap = np.inf
    for i in range(len(llr)):
        rows = S.scl_list(code, llr[i], L)
        w = S.best(rows)
        pm_sent = S.forced_path_metric(code, llr[i], S.word(code, sent[i]))
        err = not (w["info"] == sent[i]).all()
        miss = not any((r["info"] == sent[i]).all() for r in rows)
        undet = err and w["crc_ok"]
        ml = undet and w["pm"] <= pm_sent
        c += np.array([1, err, miss, undet, ml], np.uint64)
        if err:
            gap = min(gap, abs(w["pm"] - pm_sent) / max(1.0, abs(pm_sent)))
    return c, gap


_cache = {}


def reference(case):
    """(oracle, code, llr, sent, counters, gap) of one of STATS_CASES, computed once per process."""
    if case not in _cache:
        n, K, crc, L = case
        o = oracle(n, K, crc)
        code = S.Code(o)
        llr, sent = stats_inputs(o)
        _cache[case] = (o, code, llr, sent) + classify(code, llr, sent, L)
    return _cache[case]
