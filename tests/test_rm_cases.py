"""CPU: the conditions tests/test_gpu_rm_compose.py relies on hold on the recovered rows of tests/rm_cases.py — rows with exact +0.0
at punctured positions, 1000.0 at known ones and sums at repeated ones, on designs whose forced leaves end the tree. Each cap is an
assertion; the kept counts, the stage histogram and the measured SCAN deviation are printed per code (pytest -s).

Observed with the mirrors alone, the seven codes in rm_cases.KEYS order ((7, 32, 8) NR, which punctures, is the sixth):
  TieError at L = 4 / 8: 0 of 48 rows on every code (and none at 1 / 4 / 32 on the rows the adaptive schedule reaches)
  adaptive stage histogram: [21, 4, 23], [17, 12, 19], [15, 17, 16], [17, 15, 16], [16, 16, 16], [14, 15, 19], [13, 18, 17]
  flip rows kept: 48 of 48 on every code; n_dec histogram 1 .. 5: [21, 1, 2, 4, 20], [17, 6, 4, 1, 20], [15, 6, 6, 3, 18],
      [17, 3, 1, 2, 25], [16, 4, 6, 3, 19], [14, 7, 2, 2, 23], [13, 5, 1, 7, 22]
  SCAN margin rows kept: 48, 48, 45, 41, 47, 42, 44
  SCAN deviation under the perturbation, four draws: 1.2e-12, 1.1e-12, 7.6e-12, 1.6e-11, 9.0e-12, 4.8e-11, 1.0e-11
  guard model: input_guard flags all 48 rows of the three codes with punctured positions and none elsewhere; the all-frozen sum flags
      all 48 rows of the three shortening codes at list size 1; no row is within the model's spare of a criterion"""
import numpy as np
import pytest

import mask_cases as MC
import rm_cases as RC
import scl_list_numpy as S

IDS = [RC.name(k) for k in RC.KEYS]


def test_the_table_is_test_gpu_rm_s(oracle_built):
    import test_gpu_rm as T
    for key, ebno in RC.CODES.items():
        assert T.SHAPES[key][8] == ebno and T.PHI_DX == RC.PHI_DX and T.SEED == RC.SEED
    assert len(RC.KEYS) == 7


@pytest.mark.parametrize("key", RC.KEYS, ids=IDS)
def test_rows_carry_the_special_values(oracle_built, key):
    """+0.0 exactly at punctured positions, 1000.0 exactly at known ones, a sum of two received values at a doubled one; the forced
    leaves are frozen; scan_numpy.forced_coded_bits is the known set."""
    import scan_numpy as N
    c = RC.case(key)
    rx, llr, info = c.rows()
    assert llr.shape == (RC.ROWS, c.N) and rx.shape == (RC.ROWS, c.E)
    assert (llr[:, c.punctured].view(np.uint64) == 0).all() and (llr[:, c.known != 0] == 1000.0).all()
    sent = ~c.punctured & (c.known == 0)
    assert np.isfinite(llr).all() and (llr[:, sent] != 0).all()
    cnt = np.bincount(c.sel, minlength=c.N)
    for p in np.flatnonzero(cnt == 2):
        e = np.flatnonzero(c.sel == p)
        assert (llr[:, p] == (0.0 + rx[:, e[0]]) + rx[:, e[1]]).all()
    assert (c.scheme == "repeat") == bool((cnt == 2).any()) and cnt.max() <= 2
    assert (c.frozen()[c.d["forced"] != 0] == 1).all()
    forced = N.forced_coded_bits(RC.code(key))
    assert (forced == (c.known != 0)).all()
    print(c, "punctured", int(c.punctured.sum()), "known", int((c.known != 0).sum()), "doubled", int((cnt == 2).sum()),
          "fixed coded bits", int(forced.sum()))
    assert int(forced.sum()) == {("shorten", 5): 8, ("shorten", 7): 28, ("nr", 7): 28 if c.K == 56 else 0}.get((c.scheme, c.n), 0)


@pytest.mark.parametrize("key", RC.KEYS, ids=IDS)
def test_list_rows(oracle_built, key):
    """scl_list raises TieError on at most a quarter of the rows at L = 4 and 8; the mirror's best survivor is the oracle's word."""
    c = RC.case(key)
    lists, kept = RC.list_rows(key, RC.LIST_LS)
    print(c, "list rows kept", len(kept), "of", RC.ROWS)
    assert 4 * len(kept) >= 3 * RC.ROWS
    llr = c.rows()[1]
    for L in RC.LIST_LS:
        want = c.oracle().decode_scl_llr(llr[kept], L)
        got = np.stack([S.best(lists[L][i])["info"] for i in kept])
        assert (got == want).all()


@pytest.mark.parametrize("key", RC.KEYS, ids=IDS)
def test_adaptive_rows(oracle_built, key):
    """adaptive_numpy.adaptive under (1, 4, 32) delivers from all three stages."""
    kept, (info, pm, stage, ok) = RC.adaptive_reference(key)
    hist = np.bincount(stage, minlength=3).tolist()
    print(RC.case(key), "adaptive rows kept", len(kept), "stage histogram", hist, "accepted", int(ok.sum()))
    assert 4 * len(kept) >= 3 * RC.ROWS and min(hist) > 0


@pytest.mark.parametrize("key", RC.KEYS, ids=IDS)
def test_flip_rows(oracle_built, key):
    """mask_cases.flip_rows' margins keep three quarters of the rows; flip_numpy.decode at 4 flips raises no MarginError on them and
    its n_dec takes every value 1 .. 5."""
    import flip_numpy as F
    keep = RC.flip_keep(key)
    llr = RC.case(key).rows()[1][keep]
    r = F.decode(RC.code(key), llr, max(RC.FLIP_T))
    F.decode(RC.code(key), llr, 0)
    hist = np.bincount(r["n_dec"], minlength=6).tolist()
    print(RC.case(key), "flip rows kept", int(keep.sum()), "n_dec histogram", hist, "shares", F.shares(r))
    assert 4 * int(keep.sum()) >= 3 * RC.ROWS
    assert all(hist[v] > 0 for v in range(1, 6)) and hist[0] == 0


@pytest.mark.parametrize("key", RC.KEYS, ids=IDS)
def test_scan_rows(oracle_built, key):
    """The exact model's margin keeps three quarters of the rows; no NaN in the soft outputs of the exact or the min-sum model on any
    row; ext is +inf exactly at the known positions and finite at every punctured one."""
    import scan_numpy as N
    c, code = RC.case(key), RC.code(key)
    llr = c.rows()[1]
    keep = RC.scan_keep(key)
    print(c, "scan rows kept", int(keep.sum()), "of", RC.ROWS)
    assert 4 * int(keep.sum()) >= 3 * RC.ROWS
    for it in N.ITERS:
        for ms in (False, True):
            r = N.decode(code, llr, it, minsum=ms, check=False)
            assert not np.isnan(r["info_llr"]).any() and not np.isnan(r["ext"]).any()
            assert (np.isposinf(r["ext"]) == (c.known != 0)).all() and np.isfinite(r["ext"][:, c.punctured]).all()
        N.decode(code, llr[keep], it, margin=MC.SCAN_MARGIN)              # (MarginError otherwise)


def test_scan_tolerance(oracle_built):
    """mask_cases.measure_scan_tol's measurement on the margin rows of these seven codes, four draws: ten times the largest deviation
    stays below mask_cases.SCAN_TOL, which is therefore the tolerance of the GPU comparison; the figure next to
    rm_cases.SCAN_DEV_MEASURED is this one."""
    worst = {}
    for key in RC.KEYS:
        worst[RC.name(key)] = RC.measure_scan_dev(key)
        print(RC.name(key), "largest SCAN deviation under the perturbation %.3g" % worst[RC.name(key)])
    top = max(worst.values())
    print("largest of all: %.3g; recorded %.3g; SCAN_TOL %.3g" % (top, RC.SCAN_DEV_MEASURED, MC.SCAN_TOL))
    assert 10 * top <= MC.SCAN_TOL
    assert top <= 3 * RC.SCAN_DEV_MEASURED                                 # (the record is of this measurement; draws move it a little)


@pytest.mark.parametrize("key", RC.KEYS, ids=IDS)
def test_guard_model_on_recovered_rows(oracle_built, key):
    """What guard_numpy says of these rows: input_guard flags every row of a code with punctured positions and none otherwise; a
    known position puts 1000 into an all-frozen node, so the list-size-1 criterion (sum above 690) flags every row of a shortening
    code; the vectorised margins equal l1_margins row by row."""
    import guard_numpy as GN
    c, gd = RC.case(key), RC.guard(key)
    llr = c.rows()[1]
    assert (gd.bad_in == bool(c.punctured.any())).all() and not gd.tiny.any()
    if (c.known != 0).any():
        assert (gd.fsum >= 1000.0).all() and gd.flag_l1.all()
    u, _ = MC.sc_pass(RC.code(key), llr)
    for i in (0, 17, 47):
        prod, fsum, zero, win = GN.l1_margins(RC.code(key), llr[i], u[i])
        assert prod == gd.prod[i] and fsum == gd.fsum[i] and zero == gd.zero[i] and win.min() == gd.win[i]
    print(c, "model: list-size-1 set", int(gd.flag_l1.sum()), "near", int(gd.near_l1.sum()), "list set", int(gd.flag_list.sum()),
          "near", int(gd.near_list.sum()))
