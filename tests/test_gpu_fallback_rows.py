"""GPU suite: WHICH rows the fast decode families hand to the fallback pass. Every fast family (Sc8, ScLat, the exp-domain ListLat,
BatchEd: polar_decode.cpp) computes in exp-domain arithmetic, flags the codewords whose decisions it cannot guarantee and has the
LLR-domain kernel decode those again. The parity tests see the bits after that pass only: a kernel that flags every row (its own
arithmetic is then never compared with anything) or that fails to flag a row it must flag (no synthetic row lands in a window one
part in 1e10 wide) passes them all.

polar_debug_fallback_rows (include/polar_amd_debug.h) makes the fallback set observable. Here it must equal, per family and variant,
EXACTLY the rows that tests/guard_numpy.py plants on the flagged side of a criterion — and the rows planted just on the other side
must stay out. tests/test_guard_model.py proves on the CPU that the plants and the ordinary rows are what this file takes them for.
Every call also asserts the bits of EVERY row against the oracle (the tiny row, which the reference decides at the rounding noise of
its own arithmetic, against the LLR-domain kernel instead), and what ran ("lat_waves", "head_phi"). Device-pointer entry points
only."""
import ctypes as C

import numpy as np
import pytest

import guard_numpy as G

pytestmark = pytest.mark.gpu

SMALL, MID, LARGE = (7, 64, 8), (9, 256, 8), (11, 1024, 16)
KNOBS = ("lat_max_b", "lat_grid", "sc_no_fold", "no_fuse_front", "no_prefix", "no_tables", "no_head", "head_min_b")


class _Case:
    """A code of guard_numpy's table: oracle, handle, base rows; the oracle's bits of the base rows and of the planted rows, computed
    once per (format, list size) and never changed."""

    def __init__(self, key):
        import polar_amd
        from oracle_lib import Oracle
        n, K, crc = key
        self.N, self.K = 1 << n, K
        self.o = Oracle(n, K, G.EPS, crc, srand=1)
        C.CDLL(None).srand(C.c_uint(1))
        self.g = polar_amd.PolarCode(n, K, G.EPS, crc)
        assert self.g.weak_leaves == 0
        self.base = G.base_rows(self.o, key)
        self._want = {}

    def want(self, rows, fmt, L, b, tag):
        """The oracle's bits of `rows` [b][N]: those of the unplanted rows once per (format, list size, b), the planted rows' on top."""
        k = (fmt, L, b)
        if k not in self._want:
            self._want[k] = self.o.decode_scl_llr(G.widen(G.narrow(self.base[:b], fmt)), L)
            self._want[k].setflags(write=False)
        if tag is None:
            return self._want[k]
        k2 = (fmt, L, b, tag)
        if k2 not in self._want:
            w = self._want[k].copy()
            pos = list(G.planted_positions(b))
            w[pos] = self.o.decode_scl_llr(G.widen(rows[pos]), L)
            w.setflags(write=False)
            self._want[k2] = w
        return self._want[k2]


_cases = {}


def _case(key):
    if key not in _cases:
        _cases[key] = _Case(key)
    return _cases[key]


def _decode(c, rows, fmt, L, pm=False):
    """One call of the device-pointer entry point, synchronised -> (bits, the fallback set or None)."""
    import torch
    flat = np.ascontiguousarray(rows)
    t = torch.from_numpy(flat.view(np.int16) if flat.dtype in (np.uint16, np.float16) else flat).cuda()
    b = rows.shape[0]
    out = torch.zeros((b, c.K), dtype=torch.uint8, device="cuda")
    d_pm = torch.zeros(b, dtype=torch.float64, device="cuda") if pm else None
    if fmt == "f64":
        c.g.decode_scl_llr_dev(t.data_ptr(), b, L, out.data_ptr(), d_pm.data_ptr() if pm else 0)
    else:
        c.g.decode_scl_llr_dev_fmt(t.data_ptr(), fmt, b, L, out.data_ptr(), d_pm.data_ptr() if pm else 0)
    torch.cuda.synchronize()
    return out.cpu().numpy(), c.g.debug_fallback_rows()


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


def _mode1_bits(c, rows, fmt, L):
    with _forced(c, {"mode": 1, "lat_max_b": -1}):
        bits, fb = _decode(c, rows, fmt, L)
    assert fb is None                      # (the LLR-domain kernel flags nothing: no fallback pass)
    return bits


def _check(key, L, knobs, lat, head=False, fmt="f64", b=None, only=None):
    """Every planted batch of the code and format through one family and variant: the fallback set is exactly the planted set, every
    row's bits are the oracle's, and the kernel that the variant means ran."""
    c = _case(key)
    b = c.base.shape[0] if b is None else b
    batches = G.batches(c.N, fmt)
    for k, batch in enumerate(batches):
        if only is not None and k not in only:
            continue
        rows, expect = G.planted(c.base[:b], batch, L, fmt)
        want = c.want(rows, fmt, L, b, k)
        with _forced(c, knobs):
            bits, fb = _decode(c, rows, fmt, L)
            waves, phi = c.g.debug_get("lat_waves"), c.g.debug_get("head_phi")
        assert (waves > 0) == lat and (phi > 0) == head, (waves, phi)
        assert "lat_grid" not in knobs or waves == knobs["lat_grid"]
        print(f"{key} L={L} {fmt} {knobs} batch {k}: fallback set {None if fb is None else fb.tolist()}, planted {expect.tolist()}")
        assert fb is not None and fb.dtype == np.uint32 and np.array_equal(fb, expect), \
            (k, batch, None if fb is None else fb.tolist(), expect.tolist())
        tiny = [r for r, pl in zip(G.planted_positions(b), batch) if pl.kind == "tiny" and pl.flagged(L)]
        if tiny:
            want = want.copy()
            want[tiny] = _mode1_bits(c, rows, fmt, L)[tiny]
        bad = np.nonzero((bits != want).any(axis=1))[0]
        assert bad.size == 0, f"rows {bad.tolist()} of batch {k} differ from the oracle"


# ---- list size 1 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["f64", "f32", "f16", "bf16"])
@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("key", [MID, SMALL])
def test_sc8(built_lib, oracle_built, key, fold, fmt):
    """The eight-lanes-per-codeword kernel: its conversion pass (sc8_front_kernel, "sc_no_fold") and the in-place top-layer loads."""
    _check(key, 1, {"lat_max_b": -1, "sc_no_fold": 1 - fold}, lat=False, fmt=fmt)


@pytest.mark.parametrize("key", [SMALL, MID])
def test_sc_lat(built_lib, oracle_built, key):
    """sc_lat_kernel at the default grid, and three waves over 14 rows: a flagged row is followed by ordinary ones in the same wave."""
    _check(key, 1, {}, lat=True)
    _check(key, 1, {"lat_grid": 3}, lat=True, b=14)


# ---- the lists ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["f64", "f16"])
@pytest.mark.parametrize("grid", [0, 3])
@pytest.mark.parametrize("L", [2, 4, 8])
@pytest.mark.parametrize("key", [SMALL, MID])
def test_list_lat(built_lib, oracle_built, key, L, grid, fmt):
    """The exp-domain one-codeword-per-wave form of the list kernel, groups of 2 (no path metric asked for), 4 and 8 lanes."""
    _check(key, L, {"lat_grid": grid} if grid else {}, lat=True, fmt=fmt)


ED_VARIANTS = {"fused": {}, "front": {"no_fuse_front": 1}, "no_prefix": {"no_prefix": 1}, "pipe": {"tuning": (8, 0)}}


@pytest.mark.parametrize("variant", list(ED_VARIANTS))
@pytest.mark.parametrize("L", [4, 8, 16, 32])
def test_batch_ed(built_lib, oracle_built, L, variant):
    """The exp-domain batch kernel: the channel converted by the prefix kernel's fused front or by ed_front_kernel, the all-frozen
    prefix by its pass or leaf by leaf, the register-double-buffered geometry."""
    _check(MID, L, dict(ED_VARIANTS[variant], lat_max_b=-1), lat=False)


LARGE_VARIANTS = {"default": ({}, False), "tables": ({"tuning": (16, 0)}, False), "no_tables": ({"tuning": (16, 0), "no_tables": 1}, False),
                  "head": ({"tuning": (16, 0), "head_min_b": 1}, True), "no_head": ({"tuning": (16, 0), "head_min_b": 1, "no_head": 1}, False)}


@pytest.mark.parametrize("variant", list(LARGE_VARIANTS))
def test_batch_ed_large_code(built_lib, oracle_built, variant):
    """N = 2048, list of 32, 40 rows: the small-batch geometry, table mode and its absence, the two-phase head and its absence."""
    knobs, head = LARGE_VARIANTS[variant]
    _check(LARGE, 32, knobs, lat=False, head=head)


# ---- no fallback pass -------------------------------------------------------------------------------------------------------------

def test_families_without_a_fallback_pass(built_lib, oracle_built):
    """Mode 1 at a list of 4 and list size 1 with a path metric take the LLR-domain batch kernel: the hook says None (and not an
    empty or a stale set: a call with a fallback pass comes first), the bits are the oracle's."""
    c = _case(MID)
    rows, expect = G.planted(c.base, G.batches(c.N)[0], 4)
    for L, knobs, pm in ((4, {"mode": 1}, False), (1, {}, True)):
        with _forced(c, {"lat_max_b": -1}):
            _, fb = _decode(c, rows, "f64", 4)
        assert np.array_equal(fb, expect)
        with _forced(c, knobs):
            bits, fb = _decode(c, rows, "f64", L, pm=pm)
        assert fb is None
        assert (bits == c.want(rows, "f64", L, rows.shape[0], 0)).all()


# ---- flags left behind -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,L,knobs,lat", [("Sc8", 1, {"lat_max_b": -1}, False), ("BatchEd", 8, {"lat_max_b": -1}, False),
                                                ("ListLat", 4, {}, True)])
def test_flags_do_not_outlive_their_call(built_lib, oracle_built, family, L, knobs, lat):
    """One handle, three calls in a row: the planted batch, 20 ordinary rows, the planted batch again — exact, empty, exact (Sc8 keeps
    flag WORDS that it zeroes per call, the other two flag BYTES that every row's kernel writes)."""
    c = _case(MID)
    rows, expect = G.planted(c.base, G.batches(c.N)[0], L)
    assert expect.size >= 3
    plain = c.base[:G.ORDINARY_B]
    with _forced(c, knobs):
        for r, e, tag in ((rows, expect, 0), (plain, np.zeros(0, np.uint32), None), (rows, expect, 0)):
            bits, fb = _decode(c, r, "f64", L)
            assert (c.g.debug_get("lat_waves") > 0) == lat
            assert fb is not None and np.array_equal(fb, e), (family, fb, e)
            assert (bits == c.want(r, "f64", L, r.shape[0], tag)).all()
