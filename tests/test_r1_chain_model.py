"""The extended CPU model of the rate-1 continuation (tests/r1_chain_model.py) against the one it extends (tests/r1_model.py) on the
rows of the GPU tests, and its figures for the headline input: how many loop iterations the two sequels remove per wave-decode
(DESIGN.md §4)."""
import numpy as np
import pytest

import r1_chain_model
import r1_model

_tests = {}


def rows(o, seed, B, snrs):
    parts, at = [], 0
    for i, s in enumerate(snrs):
        nb = (B - at) if i == len(snrs) - 1 else B // len(snrs)
        parts.append(o.synth_llr(seed, at, nb, o.snr_sqrt_linear(s))[0])
        at += nb
    return np.concatenate(parts)


@pytest.mark.parametrize("code, B, snrs", (((8, 128, 8), 40, (0.0, 4.0)), ((9, 128, 8), 40, (0.0, 4.0)), ((6, 48, 0), 21, (1.0, 6.0))),
                         ids=("8-128-8", "9-128-8", "6-48-0"))
def test_counts_of_the_gpu_test_rows(oracle_built, code, B, snrs):
    from oracle_lib import Oracle
    n, K, crc = code
    o = Oracle(n, K, 0.32, crc, srand=1)
    fr = np.asarray(o.frozen(), np.uint8)
    llr = rows(o, 777, B, snrs)
    tests = [r1_model.leaf_tests(fr, r, 32) for r in llr]
    old = r1_model.counts(fr, llr, 32)
    for rank in (True, False):
        for chain in (True, False):
            c = r1_chain_model.counts(fr, llr, 32, rank=rank, chain=chain, tests=tests)
            print(code, "rank", rank, "chain", chain, c)
            assert (c["committed"], c["discarded"]) == old
            assert (c["rank_tried"] > 0) == rank and (c["chain_tried"] > 0) == chain
    c = r1_chain_model.counts(fr, llr, 32, tests=tests)
    assert min(r1_chain_model.six(c)[2:]) > 0, c
    assert c["rank_committed"] <= c["rank_tried"] and c["chain_committed"] <= c["chain_tried"]
    off = r1_chain_model.counts(fr, llr, 32, rank=False, chain=False, tests=tests)
    # every commit of a sequel removes loop iterations: three per quad entered after a ranking step, four per chained quad
    # (of which three were already removed by the continuation of the loop's own step at leaf 4)
    assert off["iterations"] - c["iterations"] == 3 * c["rank_committed"] + c["chain_committed"]
    assert off["ranking"] == c["ranking"]


def test_headline_figures(oracle_built):
    """(11, 1024, 0.32, 16), 48 rows at 2 dB, list of 32, leaves from the hand-over leaf 432 on, per wave-decode (24 waves)."""
    from oracle_lib import Oracle
    o = Oracle(11, 1024, 0.32, 16, srand=1)
    fr = np.asarray(o.frozen(), np.uint8)
    llr = o.synth_llr(2024, 0, 48, o.snr_sqrt_linear(2.0))[0]
    tests = [r1_model.leaf_tests(fr, r, 32) for r in llr]
    rb = r1_model.marks(fr, r1_model.weak_leaves(fr))
    assert (rb == 3).sum() == 77 and (rb == 2).sum() == 77 + 40
    per = {}
    for name, rank, chain in (("today", False, False), ("rank", True, False), ("both", True, True)):
        c = r1_chain_model.counts(fr, llr, 32, rb, start=432, rank=rank, chain=chain, tests=tests)
        per[name] = {k: v / 24.0 for k, v in c.items()}
        print(name, per[name])
    near = lambda x, want: abs(x - want) <= 0.04 * want
    assert near(per["today"]["iterations"], 654) and near(per["rank"]["iterations"], 524) and near(per["both"]["iterations"], 458)
    for name in per:
        assert near(per[name]["ranking"], 273)
    assert near(per["today"]["committed"], 128)
    assert near(per["rank"]["rank_tried"], 66) and near(per["rank"]["rank_committed"], 43.5)
    assert near(per["both"]["chain_tried"], 66.3) and near(per["both"]["chain_committed"], 65.7)
