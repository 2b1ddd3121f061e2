"""The CPU model of tests/r1_model.py extended by the two sequels of the rate-1 quad continuation (polar_amd/csrc/polar_scl_leaf.inc,
DESIGN.md §3):
  rank    the continuation is also entered after a first leaf that took the RANKING path, provided the list was full before the step
          (2^t >= L, t the number of unfrozen leaves before the leaf: the list doubles at every unfrozen leaf until it is full);
          its tests on the leaves 1 .. 3 are the same, the value of leaf 0 plays no part (the g-nodes get the bits really taken);
  chain   after a quad commit at a leaf marked rb == 3, by either entry, the second quad of the octet is tried in the same step:
          the high-word test on leaf 4 and on the leaves 5 .. 7, none of them exactly 0.
Per launch (waves of two consecutive codewords, every test ANDed over both) the model states the six counters of the test library
and the loop iterations at unfrozen leaves:
  committed        quads finished whose own first leaf passed its test: in the loop after a fast first leaf, or as a chained second quad
  discarded        continuations tried in the loop after a fast first leaf and given up
  rank_tried / rank_committed, chain_tried / chain_committed
  iterations       loop iterations at unfrozen leaves, ranking: those of them that take the ranking path, bodies: continuation bodies
                   run (first quads tried by either entry, plus chains tried)
  rank_then_chain  octets finished in one step whose first leaf took the ranking path (no device counter: what a test input is for)
A chain that gives up counts nowhere else: the loop's own step at leaf 4 then counts as before, so committed / discarded are those of
r1_model.counts whatever the switches."""
import numpy as np

import r1_model

KEYS = ("committed", "discarded", "rank_tried", "rank_committed", "chain_tried", "chain_committed", "iterations", "ranking", "bodies",
        "rank_then_chain")


def full_before(frozen, L):
    """bool per leaf: the list is full before the step (2^t >= L)."""
    frozen = np.asarray(frozen, np.uint8)
    t = np.concatenate([[0], np.cumsum(frozen == 0)])[:-1]
    return (2.0 ** np.minimum(t, 62)) >= L


def walk(frozen, tests, L, rb, start=0, rank=True, chain=True, finished=None):
    """One launch whose per-codeword leaf tests (r1_model.leaf_tests) are `tests`, walked from leaf `start` -> dict of KEYS.
    finished: a list that receives (the wave's first row, first leaf, "quad" | "chain") per block finished in one step — "chain": the
    second quad of the octet at that leaf, finished in the step of the first."""
    frozen = np.asarray(frozen, np.uint8)
    N = len(frozen)
    full = full_before(frozen, L)
    c = dict.fromkeys(KEYS, 0)
    for w in range(0, len(tests), 2):
        cws = tests[w:w + 2]

        def later(a, b):
            return all(h[a:b].all() and not z[a:b].any() for _, h, z in cws)
        phi = start
        while phi < N:
            if frozen[phi]:
                phi += 1
                continue
            c["iterations"] += 1
            fast = all(f[phi] for f, _, _ in cws)
            c["ranking"] += 0 if fast else 1
            done = ranked = False
            if rb[phi] and fast:
                c["bodies"] += 1
                if later(phi + 1, phi + 4) and not any(z[phi] for _, _, z in cws):
                    c["committed"] += 1
                    done = True
                else:
                    c["discarded"] += 1
            elif rb[phi] and rank and full[phi]:
                c["bodies"] += 1
                c["rank_tried"] += 1
                if later(phi + 1, phi + 4):
                    c["rank_committed"] += 1
                    done = ranked = True
            if not done:
                phi += 1
                continue
            if finished is not None:
                finished.append((w, phi, "quad"))
            if chain and rb[phi] == 3:
                c["bodies"] += 1
                c["chain_tried"] += 1
                if later(phi + 4, phi + 8):
                    c["chain_committed"] += 1
                    c["committed"] += 1
                    if finished is not None:
                        finished.append((w, phi, "chain"))
                    c["rank_then_chain"] += 1 if ranked else 0
                    phi += 4
            phi += 4
    return c


def counts(frozen, llr_rows, L, rb=None, start=0, rank=True, chain=True, tests=None, finished=None):
    """dict of KEYS for one launch over the rows [B, N]. `tests`: the rows' leaf tests when the caller has them already."""
    frozen = np.asarray(frozen, np.uint8)
    rb = r1_model.marks(frozen, r1_model.weak_leaves(frozen)) if rb is None else rb
    if tests is None:
        tests = [r1_model.leaf_tests(frozen, r, L) for r in np.asarray(llr_rows, np.float64)]
    return walk(frozen, tests, L, rb, start, rank, chain, finished)


def six(c):
    """the six device counters, in the order of polar_debug_get's names"""
    return tuple(c[k] for k in KEYS[:6])
