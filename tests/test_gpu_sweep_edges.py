"""GPU: the back end of a Monte-Carlo round (polar_montecarlo.cpp mc_round_launch: mc_init_alive_kernel, synth_kernel reading its
trial indices from an alive list, decode_impl with a row count that lives on the device, mc_count_compact_kernel) at its edges:
a list that runs empty with points still to come, a list that stays full, more alive trials than blocks, more trials than the
initialising grid has threads, trial indices and strides across 2^32, K that is no multiple of 64 in the bit-error count, the ASK
axis with a label tail. Each case of sweep_numpy.SWEEP_CASES is compared with the replay of the sweep rule on the oracle
(sweep_numpy.mc_reference): err, run, bit_err, and — through polar_debug_mc_alive — WHICH trials failed at the last two points, as
absolute trial indices. tests/test_sweep_model.py asserts that the cases contain the conditions named here."""
import functools

import numpy as np
import pytest

import sweep_numpy as S

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _pair(code):
    import p1_rows
    return p1_rows.pair(*code)


def _same_lists(got, want):
    """two sorted lists against two sorted lists, in either buffer order"""
    (a, b), (c, d) = got, want
    return (np.array_equal(a, c) and np.array_equal(b, d)) or (np.array_equal(a, d) and np.array_equal(b, c))


@pytest.mark.parametrize("name", list(S.SWEEP_CASES))
def test_round_equals_the_replay_on_the_oracle(built_lib, oracle_built, name):
    c = S.SWEEP_CASES[name]
    ref = S.case_reference(name)
    o, g = _pair(c["code"])
    P = ref["err"].shape
    # (the calls ADD to their accumulators)
    err, bit, run = np.full(P, 3, np.uint64), np.full(P, 5, np.uint64), np.full(P, 7, np.uint64)
    args = (c["seed"], c["t0"], c["T"], c["stride"], c["axis"], c["Ls"], c["enabled"])
    if c["call"] == "ber":
        g.mc_batch_ber(*args, err, bit, run)
        assert np.array_equal(bit - np.uint64(5), ref["bit_err"]), (bit - np.uint64(5), ref["bit_err"])
    elif c["call"] == "bicm":
        g.mc_batch_bicm(c["cid"], *args, err, run)
    else:
        g.mc_batch(*args, err, run)
    assert np.array_equal(err - np.uint64(3), ref["err"]), (err - np.uint64(3), ref["err"])
    assert np.array_equal(run - np.uint64(7), ref["run"])
    got = g.debug_mc_alive()
    want = S.last_lists(ref, c["T"], c["t0"], c["stride"], c["enabled"])
    assert got is not None and sorted(map(len, got)) == sorted(map(len, want))
    assert _same_lists(got, want), name
    if c["call"] == "ber":          # the step-wise entry point without the bit errors: the same round again, the same lists
        err2, run2 = np.zeros(P, np.uint64), np.zeros(P, np.uint64)
        g.mc_batch(*args, err2, run2)
        assert np.array_equal(err2, ref["err"]) and np.array_equal(run2, ref["run"])
        assert _same_lists(g.debug_mc_alive(), want)


def test_more_trials_than_the_initialising_grid_has_threads(built_lib, oracle_built):
    """T = 262144 + 5 on N = 4: mc_init_alive_kernel's grid-stride loop takes a second trip; counters against the oracle's own
    engine, the number of trials left alive against its error count, the alive trials themselves within the round's range"""
    c = S.INIT_CASE
    o, g = _pair(c["code"])
    T, t0, axis, seed = c["T"], c["t0"], c["axis"], c["seed"]
    en = np.ones((1, 2), np.uint8)
    e1, r1, e2, r2 = (np.zeros((1, 2), np.uint64) for _ in range(4))
    o.mc_batch(seed, t0, T, 1, axis, c["Ls"], en, e1, r1)
    g.mc_batch(seed, t0, T, 1, axis, c["Ls"], en, e2, r2)
    assert np.array_equal(e1, e2) and np.array_equal(r1, r2) and e1[0, 0] > e1[0, 1] > 0
    a, b = sorted(g.debug_mc_alive(), key=len)
    assert (len(a), len(b)) == (int(e1[0, 1]), int(e1[0, 0]))
    assert np.isin(a, b).all() and len(np.unique(b)) == len(b) and b[0] >= t0 and b[-1] < t0 + T
    assert (b >= t0 + 262144).any()          # (a trial of the second trip failed and was handed on)


def test_pipelined_driver_on_an_edge_code(built_lib, oracle_built):
    """get_bler_quick's pipelined rounds against the round-after-round loop over the device's and over the oracle's step-wise
    engine (as test_gpu_montecarlo.py's test_pipelined_rounds_equal_the_round_after_round_loop) on K = 65, with a point where
    every trial fails and points where none does: slot lists that stay full and slot lists whose count reaches 0"""
    from polar_amd.montecarlo import get_bler_quick_sharded
    c = S.PIPELINE_CASE
    o, g = _pair(c["code"])
    for max_err, batch, max_runs in c["settings"]:
        kw = dict(max_runs=max_runs, max_err=max_err, seed=c["seed"])
        _, c1 = g.get_bler_quick(c["axis"], c["Ls"], batch=batch, return_counters=True, **kw)
        _, e2, r2 = get_bler_quick_sharded(g.mc_batch, c["axis"], c["Ls"], global_batch=batch, **kw)
        assert np.array_equal(c1["err"], e2) and np.array_equal(c1["run"], r2), (max_err, batch)
        _, e3, r3 = get_bler_quick_sharded(o.mc_batch, c["axis"], c["Ls"], global_batch=batch, **kw)
        assert np.array_equal(c1["err"], e3) and np.array_equal(c1["run"], r3), (max_err, batch)
        assert (e3[:, 0] == r3[:, 0]).all() and (e3[:, -2:] == 0).all() and (r3[:, -1] == max_runs).all()
