"""CPU: the numpy models of tests/sweep_numpy.py against the oracle, and the conditions on the inputs of
tests/test_gpu_sweep_edges.py that those tests exist for — asserted here, on the model, so that a GPU test cannot pass because its
edge case never arose."""
import numpy as np
import pytest

import sweep_numpy as S


@pytest.mark.parametrize("code", sorted(set(S.FRONT_CODES + S.ASK_CODES)), ids=lambda c: "n%d_k%d_crc%d" % c)
def test_numpy_encoder_equals_the_oracle_row_by_row(oracle_built, code):
    n, K, crc = code
    o = S.make_oracle(code)
    info = S.info_rows(K, 37, 11 * n + K)
    got = S.encode(o.order(), o.crc_matrix(), n, info)
    want = np.stack([o.encode(row) for row in info])
    assert got.shape == (37, 1 << n) and np.array_equal(got, want)
    if crc:        # (the check bits matter: another CRC matrix gives another codeword for some row)
        assert not np.array_equal(S.encode(o.order(), 1 - o.crc_matrix(), n, info), want)


def test_count_errors_compares_bytes():
    a = np.zeros((4, 5), np.uint8)
    b = a.copy()
    b[1, 4] = 1
    b[3, 0] = 2
    flags, n = S.count_errors(a, b)
    assert flags.tolist() == [False, True, False, True] and n == 2


def _oracle_counters(c):
    o = S.make_oracle(c["code"])
    P = (len(c["Ls"]), len(c["axis"]))
    err, run = np.zeros(P, np.uint64), np.zeros(P, np.uint64)
    if c["call"] == "bicm":
        o.mc_batch_bicm(c["cid"], c["seed"], c["t0"], c["T"], c["stride"], c["axis"], c["Ls"], c["enabled"], err, run)
    else:
        o.mc_batch(c["seed"], c["t0"], c["T"], c["stride"], c["axis"], c["Ls"], c["enabled"], err, run)
    return err, run


@pytest.mark.parametrize("name", list(S.SWEEP_CASES))
def test_sweep_model_equals_the_oracle_engine_and_holds_its_edge(oracle_built, name):
    c = S.SWEEP_CASES[name]
    ref = S.case_reference(name)
    err, run = _oracle_counters(c)
    assert np.array_equal(ref["err"], err) and np.array_equal(ref["run"], run)
    en, T = c["enabled"], c["T"]
    assert np.array_equal(ref["run"], en.astype(np.uint64) * np.uint64(T))
    for (li, ie), f in ref["failing"].items():
        assert en[li, ie] and len(f) == ref["err"][li, ie] and np.all(f[1:] > f[:-1])
        assert np.isin(f, S.trial_indices(c["t0"], T, c["stride"])).all()
    assert ref["err"].sum() > 0 and (ref["bit_err"] >= ref["err"]).all()
    cells = [(li, ie) for li in range(en.shape[0]) for ie in range(en.shape[1]) if en[li, ie]]
    if "empty" in c["has"]:      # nobody fails, and an enabled point of the same list size follows: a launch with a row count of 0
        assert any(ref["err"][li, ie] == 0 and en[li, ie + 1:].any() for li, ie in cells)
    if "full" in c["has"]:       # the list stays full: the next enabled point reads all T entries
        assert any(ref["err"][li, ie] == T and en[li, ie + 1:].any() for li, ie in cells)
    if "last_bit" in c["has"]:   # info bit K - 1 differs in a counted trial: the tail of the lane loop over K bytes
        assert ref["last_bit"].sum() > 0
    if "cross" in c["has"]:      # failing trials below and above 2^32, also in the two lists the round leaves behind
        assert c["t0"] < 2**32 < c["t0"] + (T - 1) * c["stride"]
        for f in S.last_lists(ref, T, c["t0"], c["stride"], en):
            assert (f < 2**32).any() and (f >= 2**32).any()


def test_the_short_cases_leave_an_empty_list_behind_and_the_others_do_not(oracle_built):
    """what debug_mc_alive is compared with: two empty lists in the short-K cases, non-empty ones where trial indices matter"""
    for name, c in S.SWEEP_CASES.items():
        given, failed = S.last_lists(S.case_reference(name), c["T"], c["t0"], c["stride"], c["enabled"])
        assert np.isin(failed, given).all()
        if name.startswith("short"):
            assert len(given) == 0 and len(failed) == 0
        if name in ("cross_2_32", "compaction"):
            assert len(given) > len(failed) > 0
    assert len(S.last_lists(S.case_reference("compaction"), 8292, 0, 1, S.SWEEP_CASES["compaction"]["enabled"])[0]) > 4096


def test_the_pipelined_axis_holds_both_ends(oracle_built):
    """One round of the pipelined case on the model: all trials fail at the first point, none at the last two, for every list size —
    so the driver's slot lists run full and reach a count of 0 with a stage still to come."""
    c = S.PIPELINE_CASE
    o = S.make_oracle(c["code"])
    for max_err, batch, max_runs in c["settings"]:
        assert max_runs % batch == 0 and max_runs // batch >= 3
    T = c["settings"][0][1]
    ref = S.mc_reference(o, c["seed"], 0, T, 1, c["axis"], c["Ls"], np.ones((len(c["Ls"]), len(c["axis"])), np.uint8))
    assert (ref["err"][:, 0] == T).all() and (ref["err"][:, -2:] == 0).all() and (ref["err"][:, 1] > 0).all()


def test_a_trial_of_the_second_initialising_trip_fails(oracle_built):
    """the trials behind the first 262144 of INIT_CASE, alone: one of them fails at the first point, so the alive list that
    tests/test_gpu_sweep_edges.py reads back holds an entry that only the second trip of the initialising kernel can have written"""
    c = S.INIT_CASE
    o = S.make_oracle(c["code"])
    tail = c["T"] - 262144
    assert 0 < tail < 256
    ref = S.mc_reference(o, c["seed"], c["t0"] + 262144, tail, 1, c["axis"], c["Ls"], np.ones((1, 2), np.uint8))
    assert ref["err"][0, 0] > 0
