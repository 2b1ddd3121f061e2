"""GPU suite: `rate_recover`, then every decoder — the documented way to put rate matching in front of the list output, the adaptive,
SC-Flip and SCAN decoders, the exp-domain families and systematic=True. The rows are the recovered workload rows
of tests/rm_cases.py on seven rate-matched designs: exact +0.0 at punctured positions, 1000.0 at known ones, sums at repeated ones,
forced leaves at the end of the tree. tests/test_rm_cases.py proves on the CPU that the numpy mirrors' conditions hold on them.

Every decoder is reached twice: from host rows (`g.rate_recover(rx)`, then the call) and on the device (`rate_recover_dev` into a
torch buffer, then the decoder's `_dev` form on the same stream with nothing between the two)."""
import numpy as np
import pytest

import mask_cases as MC
import rm_cases as RC
import rm_numpy as M
import scl_list_numpy as S
from llr16_util import to_bf16_patterns, widen_bf16, widen_f16
from test_gpu_masks import FORCE_LAT, _close, _forced          # (_close: within REL = 1e-10, or the same infinity)

pytestmark = pytest.mark.gpu
IDS = [RC.name(k) for k in RC.KEYS]
SYS_KEYS = [(7, 48, 8, 100, "puncture", 2.0), (7, 48, 8, 100, "shorten", 2.0)]
_handles = {}


def _handle(key):
    if key not in _handles:
        _handles[key] = RC.case(key).handle()
    return _handles[key]


class _OnDevice:
    """The received rows on the device and rate_recover_dev into a torch buffer; the decoder's _dev call follows on the same (null)
    stream without a synchronisation."""

    def __init__(self, g, rx):
        import torch
        self.g, self.B = g, len(rx)
        self.rx = torch.from_numpy(np.array(rx, np.float64)).cuda()
        self.llr = torch.full((self.B, g.N), np.nan, dtype=torch.float64, device="cuda")

    def recover(self):
        self.g.rate_recover_dev(self.rx.data_ptr(), "f64", self.B, self.llr.data_ptr())
        return self.llr.data_ptr()

    def buffers(self, *spec):
        import torch
        return [torch.zeros(shape, dtype=getattr(torch, dt), device="cuda") for shape, dt in spec]

    @staticmethod
    def back(*tensors):
        import torch
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in tensors)


def _paths(g, rx, host, dev):
    """[("host", host(rate_recover(rx))), ("device", dev(_OnDevice))]; the recovered rows of both are the mirror's as bit patterns."""
    llr = g.rate_recover(rx)
    d = _OnDevice(g, rx)
    out = [("host", host(llr)), ("device", dev(d))]
    assert np.array_equal(llr.view(np.uint64), d.llr.cpu().numpy().view(np.uint64))
    return out


# ---- 1. the whole list ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", RC.LIST_LS)
@pytest.mark.parametrize("key", RC.KEYS, ids=IDS)
def test_whole_list(built_lib, oracle_built, key, L):
    c, g = RC.case(key), _handle(key)
    rx, llr, _ = c.rows()
    lists, kept = RC.list_rows(key, RC.LIST_LS)
    assert 4 * len(kept) >= 3 * RC.ROWS
    want_word = c.oracle().decode_scl_llr(llr, L)

    def dev(d):
        cand, pm, ok, na, win = d.buffers(((d.B, L, g.K), "uint8"), ((d.B, L), "float64"), ((d.B, L), "uint8"), ((d.B,), "int32"),
                                          ((d.B,), "int32"))
        g.decode_scl_llr_list_dev(d.recover(), "f64", d.B, L, cand.data_ptr(), pm.data_ptr(), ok.data_ptr(), na.data_ptr(), win.data_ptr())
        return d.back(cand, pm, ok, na, win)
    for path, (cand, pm, ok, na, win) in _paths(g, rx, lambda a: g.decode_scl_llr_list(a, L), dev):
        for b in kept:
            rows, a = lists[L][b], int(na[b])
            assert a == len(rows), (path, b)
            assert [x["info"].tobytes() for x in rows] == [cand[b, i].tobytes() for i in range(a)], (path, b)
            assert all(_close(pm[b, i], rows[i]["pm"]) and ok[b, i] == int(rows[i]["crc_ok"]) for i in range(a)), (path, b)
            assert (cand[b, a:] == 0).all() and np.isposinf(pm[b, a:]).all() and (ok[b, a:] == 0).all(), (path, b)
            best = S.best(rows)
            assert win[b] == [i for i, x in enumerate(rows) if x is best][0], (path, b)
        assert (win >= 0).all() and (cand[np.arange(len(rx)), win] == want_word).all(), path


# ---- 2. adaptive ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", RC.KEYS, ids=IDS)
def test_adaptive(built_lib, oracle_built, key):
    c, g = RC.case(key), _handle(key)
    kept, (info, pm, stage, ok) = RC.adaptive_reference(key)
    assert 4 * len(kept) >= 3 * RC.ROWS and len(set(stage.tolist())) == 3
    rx = c.rows()[0][kept]

    def dev(d):
        out, d_pm, st, d_ok = d.buffers(((d.B, g.K), "uint8"), ((d.B,), "float64"), ((d.B,), "uint8"), ((d.B,), "uint8"))
        g.decode_scl_llr_adaptive_dev(d.recover(), "f64", d.B, RC.ADAPTIVE, out.data_ptr(), d_pm.data_ptr(), st.data_ptr(), d_ok.data_ptr())
        return d.back(out, d_pm, st, d_ok)
    for path, got in _paths(g, rx, lambda a: g.decode_scl_llr_adaptive(a, RC.ADAPTIVE), dev):
        print(c, path, "stages", np.bincount(got[2], minlength=3).tolist(), "accepted", int(got[3].sum()), "of", len(kept))
        assert (got[0] == info).all() and (got[2] == stage).all() and (got[3] == ok).all() and _close(got[1], pm).all(), path


# ---- 3. SC-Flip -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", RC.FLIP_T)
@pytest.mark.parametrize("key", RC.KEYS, ids=IDS)
def test_sc_flip(built_lib, oracle_built, key, T):
    import flip_numpy as F
    c, g = RC.case(key), _handle(key)
    keep = RC.flip_keep(key)
    assert 4 * int(keep.sum()) >= 3 * RC.ROWS
    rx, llr = c.rows()[0][keep], c.rows()[1][keep]
    r = F.decode(RC.code(key), llr, T)

    def dev(d):
        out, ok, nd, flip, cand, mag = d.buffers(((d.B, g.K), "uint8"), ((d.B,), "uint8"), ((d.B,), "uint8"), ((d.B,), "int32"),
                                                 ((d.B, max(T, 1)), "int32"), ((d.B, max(T, 1)), "float64"))
        g.decode_sc_flip_dev(d.recover(), "f64", d.B, T, out.data_ptr(), ok.data_ptr(), nd.data_ptr(), flip.data_ptr(),
                             cand.data_ptr() if T else 0, mag.data_ptr() if T else 0)
        got = d.back(out, ok, nd, flip, cand, mag)
        return got[:4] + (got[4][:, :T], got[5][:, :T])
    for path, (out, ok, nd, flip, cand, mag) in _paths(g, rx, lambda a: g.decode_sc_flip(a, T, return_candidates=True), dev):
        print(c, path, T, "shares", F.shares(dict(info=out, crc_ok=ok, n_dec=nd)), "numpy", F.shares(r))
        assert (out == r["info"]).all() and (ok == r["crc_ok"]).all() and (nd == r["n_dec"]).all() and (flip == r["flip"]).all(), path
        assert (cand == r["cand"]).all(), path
        fin = np.isfinite(r["mag"])
        assert (np.isposinf(mag) == ~fin).all() and _close(mag[fin], r["mag"][fin]).all(), path


# ---- 4. SCAN ----------------------------------------------------------------------------------------------------------------------------
def _scan_dev(g, it, minsum):
    def dev(d):
        out, il, ext, ok, nit = d.buffers(((d.B, g.K), "uint8"), ((d.B, g.K), "float64"), ((d.B, g.N), "float64"), ((d.B,), "uint8"),
                                          ((d.B,), "uint8"))
        g.decode_scan_dev(d.recover(), "f64", d.B, it, out.data_ptr(), il.data_ptr(), ext.data_ptr(), ok.data_ptr(), nit.data_ptr(),
                          minsum=minsum)
        return d.back(out, il, ext, ok, nit)
    return dev


@pytest.mark.parametrize("key", RC.KEYS, ids=IDS)
def test_scan(built_lib, oracle_built, key):
    """1, 2 and 4 iterations: min-sum bit for bit on the first 32 rows as they come; exact mode on the margin rows with the hard
    outputs exact and the soft ones within mask_cases.SCAN_TOL (ten times the deviation tests/test_rm_cases.py measures on these
    codes is far below it); ext = +inf exactly at the known positions and finite at every punctured one."""
    import scan_numpy as N
    c, g, code = RC.case(key), _handle(key), RC.code(key)
    rx, llr, _ = c.rows()
    keep = RC.scan_keep(key)
    assert 4 * int(keep.sum()) >= 3 * RC.ROWS
    known = c.known != 0
    for it in N.ITERS:
        r = N.decode(code, llr[:RC.SCAN_ROWS], it, minsum=True)
        for path, (out, info_llr, ext, ok, nit) in _paths(g, rx[:RC.SCAN_ROWS], lambda a: g.decode_scan(a, it, minsum=True),
                                                          _scan_dev(g, it, True)):
            assert np.array_equal(out, r["info"]) and np.array_equal(ok, r["crc_ok"]) and (nit == it).all(), path
            assert np.array_equal(info_llr, r["info_llr"]) and np.array_equal(ext, r["ext"]), path
            assert (np.isposinf(ext) == known).all() and np.isfinite(ext[:, c.punctured]).all(), path
        r = N.decode(code, llr[keep], it, margin=MC.SCAN_MARGIN)
        for path, (out, info_llr, ext, ok, nit) in _paths(g, rx[keep], lambda a: g.decode_scan(a, it), _scan_dev(g, it, False)):
            dev = max(float(np.abs(np.where(np.isfinite(w), a - np.where(np.isfinite(w), w, 0), 0)).max())
                      for a, w in ((info_llr, r["info_llr"]), (ext, r["ext"])))
            print(c, path, it, "largest deviation %.3g (tolerance %.3g)" % (dev, MC.SCAN_TOL), "crc_ok", int(ok.sum()))
            assert np.array_equal(out, r["info"]) and np.array_equal(ok, r["crc_ok"]) and (nit == it).all(), path
            assert (out == (info_llr < 0)).all(), path
            assert N.same_soft(info_llr, r["info_llr"], MC.SCAN_TOL) and N.same_soft(ext, r["ext"], MC.SCAN_TOL), path
            assert (np.isposinf(ext) == known).all() and np.isfinite(ext[:, c.punctured]).all(), path


# ---- 5. the exp-domain families and the list-size-1 kernels --------------------------------------------------------------------------------
def _expected_set(key, L, B, lat):
    """(the rows of a batch of B tiled rows the model flags, the rows it cannot call) or None where the family has no fallback pass.
    List size 1 takes the pruned SC kernels (input, product and sum criteria), 8 and 32 the exp-domain kernels (input criteria and
    the windows of every path). A list of 2 decodes in LLR-domain arithmetic in every mode (choose_family): the batch kernel flags
    nothing, the one-codeword-per-wave kernel applies the input criteria of its prologue and has no windows (DESIGN.md §3 "Which rows
    take the fallback pass")."""
    gd = RC.guard(key)
    if L == 2:
        if not lat:
            return None
        flag, near = gd.flag_list, np.zeros(RC.ROWS, bool)
    else:
        flag, near = (gd.flag_l1, gd.near_l1) if L == 1 else (gd.flag_list, gd.near_list | RC.list_near(key, L))
    idx = np.arange(B) % RC.ROWS
    return set(np.flatnonzero(flag[idx]).tolist()), set(np.flatnonzero(near[idx]).tolist())


@pytest.mark.parametrize("L", [1, 2, 8, 32])
@pytest.mark.parametrize("key", RC.KEYS, ids=IDS)
def test_fast_families_on_recovered_rows(built_lib, oracle_built, key, L):
    """decode_scl_llr_dev on recovered rows in mode 0 and mode 2 — what g.decode_scl_llr(g.rate_recover(rx), L) reaches —, the batch
    kernels at B = 1000 (the 48 rows tiled) and the one-codeword-per-wave kernels at B = 48: every row equals the oracle, and the
    fallback set is the set guard_numpy's criteria give (every row of a code with punctured positions; at list size 1 every row of a
    shortening code as well: a known position puts 1000 into an all-frozen node)."""
    import torch
    c, g = RC.case(key), _handle(key)
    rx, llr, _ = c.rows()
    want = c.oracle().decode_scl_llr(llr, L)
    plain = not (c.punctured.any() or (c.known != 0).any())
    assert (g.decode_scl_llr(g.rate_recover(rx), L) == want).all()                     # host rows, the handle's own choice
    for mode in (0, 2):
        for vname, B, knobs in (("batch", 1000, {"lat_max_b": -1}), ("lat", RC.ROWS, {"lat_max_b": FORCE_LAT})):
            idx = np.arange(B) % RC.ROWS
            d = _OnDevice(g, rx[idx])
            out = torch.full((B, g.K), 7, dtype=torch.uint8, device="cuda")
            with _forced(g, dict(knobs, mode=mode)):
                g.decode_scl_llr_dev(d.recover(), B, L, out.data_ptr())
                torch.cuda.synchronize()
                fb, waves = g.debug_fallback_rows(), g.debug_get("lat_waves")
            bad = np.flatnonzero((out.cpu().numpy() != want[idx]).any(axis=1))
            assert bad.size == 0, (mode, vname, bad[:8].tolist())
            exp = _expected_set(key, L, B, vname == "lat")
            print(c, "L", L, "mode", mode, vname, "lat_waves", waves, "fallback rows", None if fb is None else len(fb),
                  "model", None if exp is None else (len(exp[0]), "near", len(exp[1])))
            if L == 2:
                assert (waves > 0) == (vname == "lat"), (mode, vname, waves)
            if exp is None:
                assert fb is None or fb.size == 0, (mode, vname)
                continue
            assert fb is not None, (mode, vname)
            flagged, near = exp
            assert set(fb.tolist()) - near == flagged - near, (mode, vname)
            if c.punctured.any() or (L == 1 and (c.known != 0).any()):
                assert flagged == set(range(B))
    g.set_mode(0)
    d = _OnDevice(g, rx)
    out = torch.zeros((RC.ROWS, g.K), dtype=torch.uint8, device="cuda")
    g.decode_scl_llr_rm_dev(d.rx.data_ptr(), "f64", RC.ROWS, L, out.data_ptr())
    torch.cuda.synchronize()
    fb = g.debug_fallback_rows()
    assert (out.cpu().numpy() == want).all()
    if not plain:
        assert fb is None                                       # (the dispatch rule: the LLR-domain family decoded the call)


# ---- 6. 16-bit received rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("key", RC.KEYS, ids=IDS)
def test_decode_rm_of_16_bit_rows(built_lib, oracle_built, key, fmt):
    """decode_scl_llr_rm(rx16, 8) and its _dev form against the oracle on recover(widen(rx16)), on every row (narrowing creates equal
    magnitudes; the oracle carries the reference's index rule and tests/test_gpu_llr16.py leaves no row out either)."""
    import torch
    c, g = RC.case(key), _handle(key)
    rx = c.rows()[0]
    if fmt == "f16":
        rx16 = rx.astype(np.float16)
        wide, host = widen_f16(rx16), g.decode_scl_llr_rm(rx16, 8)
    else:
        rx16 = to_bf16_patterns(rx)
        wide, host = widen_bf16(rx16), g.decode_scl_llr_rm(rx16, 8, fmt="bf16")
    want = c.oracle().decode_scl_llr(M.recover(wide, c.sel, c.known), 8)
    assert (g.rate_recover(rx16, fmt=fmt).view(np.uint64) == M.recover(wide, c.sel, c.known).view(np.uint64)).all()
    assert (host == want).all(), np.flatnonzero((host != want).any(axis=1))
    t = torch.from_numpy(np.ascontiguousarray(rx16).view(np.int16)).cuda()
    out = torch.full((RC.ROWS + 1, g.K), 0xA5, dtype=torch.uint8, device="cuda")
    g.decode_scl_llr_rm_dev(t.data_ptr(), fmt, RC.ROWS, 8, out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:RC.ROWS] == want).all() and (got[RC.ROWS] == 0xA5).all()
    print(c, fmt, "rows that differ from the float64 rows' words", int((want != c.oracle().decode_scl_llr(c.rows()[1], 8)).any(axis=1).sum()))


# ---- 7. systematic coding in front of rate matching -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SYS_KEYS, ids=[RC.name(k) for k in SYS_KEYS])
def test_systematic_in_front_of_rate_matching(built_lib, oracle_built, key):
    import scan_numpy as N
    import sys_numpy as SN
    import torch
    c, g, code = RC.case(key), _handle(key), RC.code(key)
    m = SN.Sys(c.n, c.K, c.crc, c.order(), c.crc_matrix())
    pos, par = g.systematic_positions()
    assert (pos == m.pos).all() and (par == m.par).all()
    # host tables: a known position is never a systematic position (its bit is 0 in every codeword, a message bit is free)
    assert not (c.known[pos] != 0).any() and not (c.known[par] != 0).any()
    msg = np.random.default_rng(7).integers(0, 2, (RC.ROWS, c.K)).astype(np.uint8)
    coded, u = g.encode_systematic(msg)
    assert (coded[:, c.known != 0] == 0).all() and (coded[:, pos] == msg).all() and (u == m.precode(msg)).all()
    clean = 8.0 * (1.0 - 2.0 * g.rate_match(coded).astype(np.float64))
    for L in (1, 8):
        assert (g.decode_scl_llr(g.rate_recover(clean), L, systematic=True) == msg).all(), L
    # the workload's rows with the systematic codeword of the trial's info bits
    rx, info = c.workload(np.arange(RC.ROWS), encode=lambda i: m.encode_systematic(i)[0])
    llr = M.recover(rx, c.sel, c.known)
    for L in (1, 8):
        u_hat = c.oracle().decode_scl_llr(llr, L)
        want = m.message(u_hat)
        assert (g.systematic_message(u_hat) == want).all()
        print(c, "L", L, "rows whose message is the sent one", int((want == info).all(axis=1).sum()), "of", RC.ROWS)
        assert (g.decode_scl_llr(g.rate_recover(rx), L, systematic=True) == want).all(), L
        d = _OnDevice(g, rx)
        out = torch.zeros((RC.ROWS, g.K), dtype=torch.uint8, device="cuda")
        g.decode_scl_llr_dev(d.recover(), RC.ROWS, L, out.data_ptr())
        g.systematic_message_dev(out.data_ptr(), RC.ROWS, out.data_ptr())
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == want).all(), L
    # SCAN: the message LLRs are llr[pos] + ext[pos] of the mirror's outputs on check 4's margin rows
    keep = RC.scan_keep(key)
    rx4, llr4 = c.rows()[0][keep], c.rows()[1][keep]
    for it in N.ITERS:
        r = N.decode(code, llr4, it, margin=MC.SCAN_MARGIN)
        out, msg_llr, ext, ok, nit = g.decode_scan(g.rate_recover(rx4), it, systematic=True)
        assert (out == m.message(r["info"])).all()
        assert N.same_soft(msg_llr, (llr4 + r["ext"])[:, pos], MC.SCAN_TOL) and N.same_soft(ext, r["ext"], MC.SCAN_TOL)
        assert np.isfinite(msg_llr).all() and not np.isposinf(msg_llr).any()
        if c.punctured[pos].any():
            assert np.array_equal(msg_llr[:, c.punctured[pos]], ext[:, pos[c.punctured[pos]]])       # (llr is +0.0 there)
