"""GPU suite: every decode family on frozen sets that no BEC construction produces (tests/mask_cases.py; DESIGN.md §2 "Non-monotone
masks"): all 254 mixed octet patterns through the pruned SC schedules and the in-register sc_block<8>, all 14 mixed quad patterns
through the flip QUAD op, the pair (unfrozen, frozen) through SCAN's PAIR op, rate-0 blocks at the very end of the walk, all-frozen
right halves beside live left siblings, a single frozen leaf inside an octet that straddles a history-word flush. Every handle comes
from PolarCode.from_tables. The rows are those the guard model keeps (tests/test_mask_cases.py proves the conditions on the CPU), so
the fast kernels decode them themselves: the fallback set is asserted empty, and "lat_waves" says which kernel ran."""
import numpy as np
import pytest

import mask_cases as MC
import scl_list_numpy as S

pytestmark = pytest.mark.gpu
REL = 1e-10          # libm against the kernel's table-driven exp / log1p: the tolerance of test_gpu_scl_list.py
KNOBS = ("lat_max_b", "sc_no_fold", "head_min_b")
FORCE_LAT = 1 << 40

_handles = {}


def _handle(tab):
    if tab.name not in _handles:
        _handles[tab.name] = tab.handle()
        assert _handles[tab.name].weak_leaves == 0
    return _handles[tab.name]


def _table(name):
    if name in MC.EDGE_NAMES:
        return MC.edge_masks()[name]
    _, n, i = name.split("-")
    return MC.octet_codes(int(n[1:]))[int(i)]


class _forced:
    """Knobs of polar_debug_set, "tuning" (set_tuning's arguments) and "mode", undone afterwards."""

    def __init__(self, g, knobs):
        self.g, self.knobs = g, dict(knobs)

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


def _decode(g, llr, L, pm=False):
    """decode_scl_llr_dev, synchronised -> (bits, metrics or None, the fallback set or None, lat_waves)."""
    import torch
    B = len(llr)
    t = torch.from_numpy(np.ascontiguousarray(llr)).cuda()
    out = torch.full((B, g.K), 7, dtype=torch.uint8, device="cuda")
    d_pm = torch.full((B,), -1.0, dtype=torch.float64, device="cuda") if pm else None
    g.decode_scl_llr_dev(t.data_ptr(), B, L, out.data_ptr(), d_pm.data_ptr() if pm else 0)
    torch.cuda.synchronize()
    return out.cpu().numpy(), d_pm.cpu().numpy() if pm else None, g.debug_fallback_rows(), g.debug_get("lat_waves")


def _close(a, b):
    """Within REL, or the same infinity (a frozen leaf whose cost overflows in the reference's arithmetic as well)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    return np.where(fin, np.abs(np.where(fin, a, 0.0) - np.where(fin, b, 0.0)) <= REL * np.maximum(1.0, np.abs(np.where(fin, b, 0.0))), a == b)


# ---- list size 1 --------------------------------------------------------------------------------------------------------------------
L1_VARIANTS = {"batch": ({"lat_max_b": -1}, False), "no_fold": ({"lat_max_b": -1, "sc_no_fold": 1}, False),
               "lat": ({"lat_max_b": FORCE_LAT}, True)}


@pytest.mark.parametrize("variant", list(L1_VARIANTS))
@pytest.mark.parametrize("name", ["octets-n%d-%d" % (n, i) for n in (11, 10) for i in range(MC.N_CODES[n])])
def test_list_size_1(built_lib, oracle_built, name, variant):
    """sc8_decode_kernel (with its conversion pass and with the in-place top-layer loads) and sc_lat_kernel on the kept rows of every
    octet-pattern code: the oracle's bits, from the fast kernel itself."""
    tab = _table(name)
    g, r = _handle(tab), MC.rows(tab)
    k = np.flatnonzero(r.keep_l1)
    knobs, lat = L1_VARIANTS[variant]
    with _forced(g, knobs):
        bits, _, fb, waves = _decode(g, r.llr[k], 1)
    print(name, variant, "rows", len(k), "block errors", int(r.err_l1[k].sum()), "lat_waves", waves, "fallback set", None if fb is None else fb.tolist())
    assert (waves > 0) == lat
    assert fb is not None and fb.size == 0
    bad = np.flatnonzero((bits != r.bits_l1[k]).any(axis=1))
    assert bad.size == 0, f"rows {k[bad].tolist()} differ from the oracle"


# ---- the list kernels ------------------------------------------------------------------------------------------------------------------
LIST_CODES = ["octets-n10-0", "octets-n10-7"] + list(MC.EDGE_NAMES)
BOTH = [("batch", {"lat_max_b": -1}, False), ("lat", {"lat_max_b": FORCE_LAT}, True)]
LIST_VARIANTS = {2: BOTH, 4: BOTH, 8: BOTH, 5: BOTH, 16: [("batch", {}, False)], 33: [("batch", {}, False)],
                 32: [("mode0", {}, False), ("mode1", {"mode": 1}, False), ("mode2", {"mode": 2}, False),
                      ("head", {"tuning": (16, 0), "head_min_b": 1}, False)]}
_want = {}


def _list_reference(tab, L):
    """Per (code, list size), once: the kept rows, the oracle's bits, the list call's winner metric (held against path_metric bit for
    bit and against the numpy forced pass here)."""
    if (tab.name, L) not in _want:
        g, r = _handle(tab), MC.rows(tab)
        k = np.flatnonzero(r.keep_list)
        llr = r.llr[k]
        want = tab.oracle().decode_scl_llr(llr, L)
        cand, pm, ok, na, win = g.decode_scl_llr_list(llr, L)
        rows = np.arange(len(k))
        assert (win >= 0).all() and (ok[rows, win] == 1).all()
        assert (cand[rows, win] == want).all(), "the list call's winner is not the oracle's word"
        pm_w = pm[rows, win]
        assert np.array_equal(pm_w.view(np.uint64), g.path_metric(llr, want).view(np.uint64))
        some = rows[:: max(1, len(rows) // 6)]
        forced = np.array([S.forced_path_metric(r.code, llr[i], S.word(r.code, want[i])) for i in some])
        assert _close(pm_w[some], forced).all(), (pm_w[some], forced)
        _want[(tab.name, L)] = (llr, want, pm_w)
    return _want[(tab.name, L)]


@pytest.mark.parametrize("L", list(LIST_VARIANTS))
@pytest.mark.parametrize("name", LIST_CODES)
def test_list_kernels(built_lib, oracle_built, name, L):
    """Lists of 2, 4, 8 and 5 through the batch kernel and the one-codeword-per-wave kernel, 16 and 33 through the batch kernel, 32
    in both arithmetics, forced exp-domain, and with the two-phase head: the oracle's bits, the winner's metric, an empty fallback
    set wherever the family has a fallback pass."""
    tab = _table(name)
    g = _handle(tab)
    llr, want, pm_w = _list_reference(tab, L)
    for vname, knobs, lat in LIST_VARIANTS[L]:
        with _forced(g, knobs):
            bits, pm, fb, waves = _decode(g, llr, L, pm=True)
            phi = g.debug_get("head_phi")
        print(name, L, vname, "rows", len(llr), "lat_waves", waves, "head_phi", phi, "fallback set", None if fb is None else fb.tolist())
        assert (waves > 0) == lat, (vname, waves)
        assert fb is None or fb.size == 0, (vname, fb)
        if L >= 3 and knobs.get("mode", 0) != 1:
            assert fb is not None, vname                         # (exp-domain arithmetic: the family has a fallback pass)
        bad = np.flatnonzero((bits != want).any(axis=1))
        assert bad.size == 0, f"{vname}: rows {bad.tolist()} differ from the oracle"
        assert _close(pm, pm_w).all(), vname
        if knobs.get("mode", 0) == 1:
            assert np.array_equal(pm.view(np.uint64), pm_w.view(np.uint64))


# ---- the whole list ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 8])
@pytest.mark.parametrize("name", [x for x in MC.EDGE_NAMES if x.startswith("d-")])
def test_whole_list(built_lib, oracle_built, name, L):
    """decode_scl_llr_list on the N = 128 masks against scl_list_numpy.scl_list: the same survivors in the same order, metrics to REL."""
    tab = _table(name)
    g = _handle(tab)
    llr, _, lists, kept = MC.list_rows(tab, (4, 8))
    assert 4 * len(kept) >= 3 * len(llr)
    cand, pm, ok, na, win = g.decode_scl_llr_list(llr, L)
    for b in kept:
        rows = lists[L][b]
        a = int(na[b])
        assert a == len(rows), b
        assert [x["info"].tobytes() for x in rows] == [cand[b, i].tobytes() for i in range(a)], b
        assert all(_close(pm[b, i], rows[i]["pm"]) and ok[b, i] == 1 for i in range(a)), b
        assert (cand[b, a:] == 0).all() and np.isposinf(pm[b, a:]).all() and win[b] == 0
    assert (cand[kept, 0] == tab.oracle().decode_scl_llr(llr[kept], L)).all()


# ---- adaptive ----------------------------------------------------------------------------------------------------------------------------
def test_adaptive(built_lib, oracle_built):
    """Schedule (1, 4, 32) on the CRC variant of an N = 128 mask against adaptive_numpy.adaptive, rows with a tie excluded on the CPU."""
    import adaptive_numpy as A
    tab = MC.adaptive_case()
    g = _handle(tab)
    llr, _, _, kept = MC.list_rows(tab, MC.ADAPTIVE)
    assert 4 * len(kept) >= 3 * len(llr)
    info, pm, stage, ok = A.adaptive(S.Code(tab), llr[kept], MC.ADAPTIVE)
    got = g.decode_scl_llr_adaptive(llr[kept], MC.ADAPTIVE)
    print("stages", np.bincount(got[2], minlength=3).tolist(), "accepted", int(got[3].sum()), "of", len(kept))
    assert (got[0] == info).all() and (got[2] == stage).all() and (got[3] == ok).all() and _close(got[1], pm).all()
    assert len(set(stage.tolist())) == 3 and 0 < ok.sum()


# ---- SC-Flip -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", MC.FLIP_T)
@pytest.mark.parametrize("i", range(MC.N_SOFT))
def test_sc_flip(built_lib, oracle_built, i, T):
    """Every output of decode_sc_flip against flip_numpy.decode on the CRC variants: words, flags, passes, flipped positions and
    candidates exactly, magnitudes to REL."""
    import flip_numpy as F
    tab = MC.soft_codes()[i]
    g = _handle(tab)
    llr, _ = MC.flip_rows(tab)
    r = F.decode(S.Code(tab), llr, T)
    out, ok, nd, flip, cand, mag = g.decode_sc_flip(llr, T, return_candidates=True)
    print(tab, T, "shares", F.shares(dict(info=out, crc_ok=ok, n_dec=nd)), "numpy", F.shares(r))
    assert (out == r["info"]).all() and (ok == r["crc_ok"]).all() and (nd == r["n_dec"]).all() and (flip == r["flip"]).all()
    assert (cand == r["cand"]).all()
    fin = np.isfinite(r["mag"])
    assert (np.isposinf(mag) == ~fin).all() and _close(mag[fin], r["mag"][fin]).all()


# ---- SCAN ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(MC.N_SOFT + 2))
def test_scan(built_lib, oracle_built, i):
    """1, 2 and 4 iterations: min-sum arithmetic bit for bit on rows as they come; exact arithmetic with the hard outputs exact and
    the soft ones within the CPU-measured SCAN_TOL on rows the model keeps; ext = +inf exactly where the frozen set fixes a bit."""
    import scan_numpy as M
    tab = MC.scan_codes()[i]
    g, code = _handle(tab), S.Code(tab)
    plain, clean = MC.scan_rows(tab)
    forced = M.forced_coded_bits(code)
    # (a coded bit is fixed only where the LAST leaf is frozen: x[N - 1] = u[N - 1], and every other fixed bit needs that one)
    assert forced.any() == bool(code.frozen[-1]) and (forced.any() or not tab.name.startswith("a-"))
    for it in M.ITERS:
        r = M.decode(code, plain, it, minsum=True)
        out, info_llr, ext, ok, nit = g.decode_scan(plain, it, minsum=True)
        assert np.array_equal(out, r["info"]) and np.array_equal(ok, r["crc_ok"]) and (nit == it).all()
        assert np.array_equal(info_llr, r["info_llr"]) and np.array_equal(ext, r["ext"])
        assert (np.isposinf(ext) == forced).all()
        r = M.decode(code, clean, it, margin=MC.SCAN_MARGIN)           # (MarginError if a hard result could depend on the tolerance)
        out, info_llr, ext, ok, nit = g.decode_scan(clean, it)
        dev = max(float(np.abs(np.where(np.isfinite(w), a - np.where(np.isfinite(w), w, 0), 0)).max())
                  for a, w in ((info_llr, r["info_llr"]), (ext, r["ext"])))
        print(tab, it, "largest deviation %.3g (tolerance %.3g)" % (dev, MC.SCAN_TOL), "crc_ok", int(ok.sum()))
        assert np.array_equal(out, r["info"]) and np.array_equal(ok, r["crc_ok"]) and (nit == it).all()
        assert (out == (info_llr < 0)).all()
        assert M.same_soft(info_llr, r["info_llr"], MC.SCAN_TOL) and M.same_soft(ext, r["ext"], MC.SCAN_TOL)
        assert (np.isposinf(ext) == forced).all()


# ---- probability domain ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["octets-n10-0", "a-last-leaf", "a-last-quad"])
def test_probability_domain(built_lib, oracle_built, name):
    """decode_sc_p1 (both kernels) and decode_scl_p1 at a list of 4 against the oracle with the same tables, the same doubles."""
    import p1_rows
    from golden_util import both_kernels
    tab = _table(name)
    g, o, r = _handle(tab), tab.oracle(), MC.rows(tab)
    llr = np.concatenate([r.llr[:12], r.llr[MC.B_POINT:MC.B_POINT + 12]])
    p1 = 1.0 / (1.0 + np.exp(llr))
    p0 = 1.0 - p1
    got = both_kernels(g, lambda: g.decode_sc_p1(p1))
    want = np.stack([o.decode_sc_p1(p1[i]) for i in range(len(p1))])
    assert p1_rows.rows_that_differ(got, want).size == 0
    got = g.decode_scl_p1(p1, p0, 4)
    want = np.stack([o.decode_scl_p1(p1[i], p0[i], 4) for i in range(len(p1))])
    assert (got == want).all()
