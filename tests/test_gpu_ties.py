"""GPU suite: rows of ONE LLR magnitude — sign(noisy codeword) * 45, what a hard-decision front end or saturated 16-bit LLRs
deliver — where almost every fork of the list walk sits on a tie and the reference's answer rests on its index rule (DESIGN.md §2
"Limit"). tests/tie_numpy.py restates that rule and tells, per row and list size, whether the row is EXACTLY DECIDED: the fp64 walk
keeps at every fork the set that exact metrics a + k log 2 keep. tests/test_tie_model.py proves the model against the oracle and
the stored indices (tests/golden/tie_rows.npz) against the model.

On the exactly decided rows everything here must equal the oracle / the model bit for bit: decode_scl_llr in every family
choose_family can reach (device and host pointers, with and without the rate-1 marks, four element formats), the list output with
its metrics as 64-bit patterns, path_metric, the adaptive decoder, SC-Flip and min-sum SCAN. On the other rows nothing is
asserted against the oracle; the number of rows that differ is printed, for the LLR-domain kernel too. Every device-pointer call
prints how many rows its fast kernel kept for itself (polar_debug_fallback_rows): a family that flags every row proves only its
fallback pass, and that must be visible."""
import ctypes as C

import numpy as np
import pytest

import tie_numpy as T

pytestmark = pytest.mark.gpu

SMALL = ((8, 128, 8), (9, 128, 8))
LARGE = ((10, 512, 8), (10, 256, 8))
CODES = SMALL + LARGE
KNOBS = ("lat_max_b", "no_r1", "no_head", "head_min_b")
ids = lambda c: "-".join(str(v) for v in c) if isinstance(c, tuple) else str(c)            # noqa: E731


class _Case:
    def __init__(self, code):
        import polar_amd
        self.code, self.K, self.N = code, code[1], 1 << code[0]
        self.o, self.c, self.x = T.case(code)
        C.CDLL(None).srand(C.c_uint(1))
        self.g = polar_amd.PolarCode(code[0], code[1], 0.32, code[2])
        assert self.g.weak_leaves == 0
        self.gold = T.load_golden()
        self._want = {}

    def want(self, L):
        """the oracle's bits, once per list size; the stored bits are the same"""
        if L not in self._want:
            self._want[L] = self.o.decode_scl_llr(self.x, L)
            self._want[L].setflags(write=False)
            assert (self._want[L] == self.gold[(self.code, L)][1]).all()
        return self._want[L]

    def exact(self, L):
        return self.gold[(self.code, L)][0]


_cases = {}


def _case(code):
    if code not in _cases:
        _cases[code] = _Case(code)
    return _cases[code]


class _forced:
    """The knobs of a variant (polar_debug_set keys; "tuning": set_tuning's arguments; "mode"), undone afterwards."""

    def __init__(self, c, knobs):
        self.g, self.knobs = c.g, dict(knobs)

    def __enter__(self):
        for k, v in self.knobs.items():
            if k == "tuning":
                self.g.set_tuning(*v)
            elif k == "mode":
                self.g.set_mode(v)
            else:
                self.g.debug_set(k, v)

    def __exit__(self, *exc):
        for k in KNOBS:
            self.g.debug_set(k, 0)
        self.g.set_tuning()
        self.g.set_mode(0)


def _decode_dev(c, L, pm=False):
    """decode_scl_llr on device pointers, synchronised -> (bits, pm or None, fallback set or None, lat_waves, head_phi)"""
    import torch
    b = c.x.shape[0]
    t = torch.from_numpy(np.ascontiguousarray(c.x)).cuda()
    out = torch.full((b, c.K), 7, dtype=torch.uint8, device="cuda")
    d_pm = torch.zeros(b, dtype=torch.float64, device="cuda") if pm else None
    c.g.decode_scl_llr_dev(t.data_ptr(), b, L, out.data_ptr(), d_pm.data_ptr() if pm else 0)
    torch.cuda.synchronize()
    return (out.cpu().numpy(), d_pm.cpu().numpy() if pm else None, c.g.debug_fallback_rows(), c.g.debug_get("lat_waves"),
            c.g.debug_get("head_phi"))


def _winner_pm(code, L, r):
    res = T.walked(code, L, r)
    return [p["pm"] for p in res.paths if p["index"] == res.winner]


# family, list sizes, knobs, a path metric asked for, the one-codeword-per-wave form, a fallback pass
FAMILIES = {
    "ScLat": ((1,), {}, False, True, True),
    "Sc8": ((1,), {"lat_max_b": -1}, False, False, True),
    "ListLat": ((2, 4, 8), {}, False, True, True),
    "BatchLlr": ((1, 2, 3, 8, 24, 32), {"mode": 1, "lat_max_b": -1}, True, False, False),
    "BatchEd": ((4, 8, 16, 24, 32), {"lat_max_b": -1}, False, False, True),
    "fat-wave": ((16, 24, 32), {}, False, False, True),                      # the default small-batch geometry
    "head": ((32,), {"tuning": (16, 0), "head_min_b": 1}, False, False, True),
    "no-head": ((32,), {"tuning": (16, 0), "head_min_b": 1, "no_head": 1}, False, False, True),
}
# the hand-over leaf of the two-phase form: (9, 128, 8) has a window of 81 leaves between the all-frozen prefix and the third
# unfrozen leaf, (10, 256, 8) one of 113 (the fixed-N instantiation of the kernel); (8, 128, 8) has no prefix pass and (10, 512, 8) a
# window of 33 < 64, so both decode in one phase
HEAD_PHI = {(8, 128, 8): 0, (9, 128, 8): 208, (10, 512, 8): 0, (10, 256, 8): 368}


def _pairs(Ls, codes=CODES):
    """(code, L) for the list sizes of Ls at which the code has its exactly decided rows stored"""
    return [(code, L) for code in codes for L in Ls if L in T.TIE_CODES[code][1]]


@pytest.mark.parametrize("code,family", [(code, f) for code in CODES for f in FAMILIES if _pairs(FAMILIES[f][0], (code,))],
                         ids=lambda v: ids(v))
def test_decode_scl_llr_families(built_lib, oracle_built, code, family):
    """Device and host pointers, with and without the rate-1 marks (list sizes above 16: the list-of-32 kernels read them)."""
    c = _case(code)
    Ls, knobs, pm, lat, has_fb = FAMILIES[family]
    b = c.x.shape[0]
    for L in Ls:
        if L not in T.TIE_CODES[code][1]:
            continue
        want, ex = c.want(L), c.exact(L)
        with _forced(c, {"mode": 1, "lat_max_b": -1}):
            ref1 = _decode_dev(c, L)[0]
        for no_r1 in ((0, 1) if L > 16 else (0,)):
            with _forced(c, dict(knobs, no_r1=no_r1)):
                bits, d_pm, fb, waves, phi = _decode_dev(c, L, pm)
                host = c.g.decode_scl_llr(c.x, L)
            kept = None if fb is None else b - len(fb)
            off = np.nonzero((bits != want).any(axis=1))[0]
            print("%s %-8s L = %2d no_r1 = %d: fast kernel kept %s of %d rows (exactly decided: %s of %d); off the oracle: rows %s "
                  "(LLR-domain kernel: %s); lat_waves %d head_phi %d" %
                  (ids(code), family, L, no_r1, kept, b, None if fb is None else len(set(ex) - set(fb.tolist())), len(ex),
                   off.tolist(), np.nonzero((ref1 != want).any(axis=1))[0].tolist(), waves, phi))
            assert (waves > 0) == lat, waves
            assert (fb is not None) == has_fb
            assert phi == (HEAD_PHI[code] if family == "head" else 0)
            assert (bits[ex] == want[ex]).all(), "exactly decided rows %s differ from the oracle" % [r for r in off if r in ex]
            assert (host[ex] == want[ex]).all(), np.nonzero((host != want).any(axis=1))[0]
            assert (ref1[ex] == want[ex]).all()
            if d_pm is not None:
                for r in ex:
                    w = _winner_pm(code, L, int(r))
                    if w and np.isfinite(w[0]):
                        assert np.float64(w[0]).view(np.uint64) == d_pm[r].view(np.uint64), (r, w[0], d_pm[r])


@pytest.mark.parametrize("code,L", _pairs((1, 8, 32)), ids=lambda v: ids(v))
def test_element_formats(built_lib, oracle_built, code, L):
    """45.0 is exact in binary16, bfloat16 and float32: the same rows in every format give the float64 call's bits, on all rows."""
    import llr16_util
    c = _case(code)
    f64 = c.g.decode_scl_llr(c.x, L)
    ex = c.exact(L)
    assert (f64[ex] == c.want(L)[ex]).all()
    f16 = c.x.astype(np.float16)
    bf = llr16_util.to_bf16_patterns(c.x)
    assert (llr16_util.widen_f16(f16) == c.x).all() and (llr16_util.widen_bf16(bf) == c.x).all()
    for name, got in (("f32", c.g.decode_scl_llr(c.x.astype(np.float32), L)), ("f16", c.g.decode_scl_llr(f16, L)),
                      ("f16 patterns", c.g.decode_scl_llr(f16.view(np.uint16), L, fmt="f16")),
                      ("bf16", c.g.decode_scl_llr(bf, L, fmt="bf16"))):
        assert (got == f64).all(), (name, np.nonzero((got != f64).any(axis=1))[0])


def _model_list(code, L, r, K):
    """(cand [L, K], pm [L], crc_ok [L], n_active, winner) of the model's final list in the row order of the header"""
    res = T.walked(code, L, r)
    rows = res.sorted_list()
    cand, pm, ok = np.zeros((L, K), np.uint8), np.full(L, np.inf), np.zeros(L, np.uint8)
    for i, p in enumerate(rows):
        cand[i], pm[i], ok[i] = p["info"], p["pm"], p["crc_ok"]
    win = [i for i, p in enumerate(rows) if p["index"] == res.winner]
    return cand, pm, ok, len(rows), (win[0] if win else -1)


@pytest.mark.parametrize("code,L", _pairs((4, 8, 32)), ids=lambda v: ids(v))
def test_list_output(built_lib, oracle_built, code, L):
    """cand, crc_ok, n_active, winner and the row order against the model's final list sorted by the header's rule (CRC pass first,
    then the smaller metric, then the lower path index); pm against the model's fp64 metrics as 64-bit patterns; path_metric of the
    returned rows gives the same patterns — of the rows with crc_ok = 1: path_metric takes the info bits and sets the check bits
    from the CRC matrix, so it prices another word than a row that failed the CRC holds."""
    c = _case(code)
    cand, pm, ok, na, win = c.g.decode_scl_llr_list(c.x, L)
    again = c.g.path_metric(c.x, cand)
    n_checked = 0
    for r in c.exact(L):
        m_cand, m_pm, m_ok, m_na, m_win = _model_list(code, L, int(r), c.K)
        assert na[r] == m_na and win[r] == m_win, (r, na[r], m_na, win[r], m_win)
        assert (ok[r] == m_ok).all() and (cand[r] == m_cand).all(), (r, np.nonzero((cand[r] != m_cand).any(axis=1))[0])
        assert (pm[r].view(np.uint64) == m_pm.view(np.uint64)).all(), (r, pm[r], m_pm)
        passed = ok[r] == 1
        assert (again[r][passed].view(np.uint64) == pm[r][passed].view(np.uint64)).all(), (r, again[r][passed], pm[r][passed])
        n_checked += int(passed.sum())
        if win[r] >= 0:
            assert (cand[r, win[r]] == c.want(L)[r]).all()
    print("%s L = %d: %d rows, %d path_metric values compared, tied final metrics in %d rows" %
          (ids(code), L, len(c.exact(L)), n_checked, sum(len(set(pm[r][:na[r]].tolist())) < na[r] for r in c.exact(L))))
    assert n_checked > 0


@pytest.mark.parametrize("code", SMALL, ids=ids)
def test_adaptive(built_lib, oracle_built, code):
    """decode_scl_llr_adaptive with (1, 4, 32) equals the list call at the accepting stage — on the rows exactly decided at every
    stage they go through, against the model's winner too."""
    c = _case(code)
    sched = (1, 4, 32)
    out, pm, stage, ok = c.g.decode_scl_llr_adaptive(c.x, sched)
    lists = {L: c.g.decode_scl_llr_list(c.x, L) for L in sched}
    seen = np.zeros(3, int)
    for r in range(c.x.shape[0]):
        s_want = next((s for s, L in enumerate(sched) if lists[L][2][r, max(lists[L][4][r], 0)] == 1), len(sched) - 1)
        if any(r not in c.exact(L) for L in sched[:s_want + 1]):
            continue
        cand, lpm, lok, _, win = (a[r] for a in lists[sched[s_want]])
        assert stage[r] == s_want and ok[r] == lok[max(win, 0)]
        assert win >= 0 and (out[r] == cand[win]).all() and pm[r].view(np.uint64) == lpm[win].view(np.uint64)
        assert (out[r] == c.want(sched[s_want])[r]).all()
        seen[s_want] += 1
    print("%s adaptive: rows delivered per stage %s" % (ids(code), seen.tolist()))
    assert seen.sum() >= c.x.shape[0] // 2


@pytest.mark.parametrize("T_flips", (0, 8))
@pytest.mark.parametrize("code", CODES, ids=ids)
def test_sc_flip(built_lib, oracle_built, code, T_flips):
    """Every magnitude is a multiple of 45: cand is decided almost wholly by "equal magnitudes by position ascending". Against
    flip_numpy on the rows whose list-of-1 walk meets no fork tie (a zero unfrozen leaf LLR: the model tells which rows). Those
    rows all pass the CRC in the first pass: the candidates and their magnitudes are what is compared, no retry runs."""
    import flip_numpy as F
    c = _case(code)
    rows = [r for r in range(c.x.shape[0]) if not T.walked(code, 1, r).tie_forks()]
    assert len(rows) >= 4, rows                             # (a property of the inputs: 5, 10, 4 and 4 rows of the four codes)
    want = F.decode(c.c, c.x[rows], T_flips, check=False)
    got = c.g.decode_sc_flip(c.x[rows], T_flips, return_candidates=True)
    print("%s T = %d: %d rows, n_dec %s, equal neighbours among the candidates' magnitudes: %d" %
          (ids(code), T_flips, len(rows), np.bincount(got[2], minlength=T_flips + 2).tolist(), int((np.diff(want["mag"], axis=1) == 0).sum())))
    for name, g_, w_ in zip(("info", "crc_ok", "n_dec", "flip", "cand", "mag"), got,
                            (want["info"], want["crc_ok"], want["n_dec"], want["flip"], want["cand"], want["mag"])):
        assert np.array_equal(g_, w_), (name, np.nonzero(np.asarray(g_ != w_).reshape(len(rows), -1).any(axis=1))[0])
    assert (np.mod(want["mag"][np.isfinite(want["mag"])], T.TIE_C) == 0).all()


@pytest.mark.parametrize("iters", (1, 4))
@pytest.mark.parametrize("code", CODES, ids=ids)
def test_scan_minsum(built_lib, oracle_built, code, iters):
    """POLAR_SCAN_MINSUM: the values are integers throughout, every output of every row bit for bit."""
    import scan_numpy as M
    c = _case(code)
    r = M.decode(c.c, c.x, iters, minsum=True)
    out, info_llr, ext, ok, nit = c.g.decode_scan(c.x, iters, minsum=True)
    assert np.array_equal(out, r["info"]) and np.array_equal(ok, r["crc_ok"]) and np.array_equal(nit, r["n_iter"])
    assert np.array_equal(info_llr, r["info_llr"]) and np.array_equal(ext, r["ext"])
    fin = np.isfinite(ext)
    assert (np.mod(ext[fin], T.TIE_C) == 0).all()
