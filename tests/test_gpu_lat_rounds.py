"""GPU suite: the later trips of the one-codeword-per-wave ("latency") kernels. Each of them keeps one codeword's whole decoder state in
a wave's LDS and registers and loops to a further codeword when the batch is larger than the launch — sc_lat_kernel, sc_p1_lat_kernel
and mlc_sc_lat_kernel with a static stride, scl_decode_llr_kernel<.., LAT = 1> from a device counter. From the second trip on,
everything the wave left behind meets a new row: bit-packed partial sums and decisions, history and origin words, the path stack,
the flag byte, the re-encoded lower levels of the MLC receiver.

Two hooks of include/polar_amd_debug.h make the trips a statement instead of an accident of the batch size: "lat_grid" caps the
blocks of such a launch (a dozen rows then drive a wave through four or five codewords at any block length, whatever the CU
count), and "lat_waves" tells how many blocks the last decode call's latency launch had — 0 when the host fell back to the batch
kernel (the state does not fit the LDS, n > 12, mode 1 with a list above 2). Every forced call here asserts that the kernel it
means to test ran, and how many trips its waves made.

Rows are the fuzzers': Oracle(n, K, 0.32, crc, srand=1).synth_llr and the three degenerate rows of fuzz_util.run_one (all-zero,
+-1000 alternating, everything x 1e-3). The degenerate rows are the only rows ever left out of the comparison with the oracle
(the reference decides them at the rounding noise of its own arithmetic); they sit below AND at or above the grid size, so that a
flagged codeword comes before and after ordinary ones in the same wave and the fallback pass has to patch the right rows. Every
comparison is equality: bits against the oracle and against the batch kernel, path metrics against the batch kernel as 64-bit
patterns, doubles (NaN positions apart) for decode_sc_p1 and the MLC receiver."""
import ctypes as C

import numpy as np
import pytest

import llr16_util
import p1_rows
from golden_util import both_kernels

pytestmark = pytest.mark.gpu

GRID, B_CAP, DEG_CAP = 3, 14, (1, 5, 9)          # the capped launches: three waves, 14 rows -> four or five rows per wave
# the four codes of tools/stress_parity_lat.py; N < 8 (the pair's operands live in registers) and N < 128 (no constant-shift walk of
# the partial sums); N = 4096, where only the groups of 1 and 2 lanes fit the LDS
CODES = [(7, 40, 0), (9, 300, 8), (10, 512, 0), (11, 1024, 16), (3, 4, 0), (5, 16, 0), (12, 2048, 0)]


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _degenerate(llr, rows):
    """The three degenerate rows of fuzz_util.run_one, in turn, at `rows`; returns the mask of the ordinary rows."""
    N = llr.shape[1]
    for k, r in enumerate(rows):
        if k % 3 == 0:
            llr[r] = 0.0
        elif k % 3 == 1:
            llr[r] = np.where(np.arange(N) % 2 == 0, 1e3, -1e3)
        else:
            llr[r] *= 1e-3
    ordinary = np.ones(llr.shape[0], bool)
    ordinary[list(rows)] = False
    return ordinary


class _Case:
    """A code, its oracle and its handle, rows with degenerate ones among them, and the oracle's bits per list size (computed once,
    never changed)."""

    def __init__(self, n, K, crc, B, ebno, seed, deg):
        import polar_amd
        from oracle_lib import Oracle
        self.n, self.N, self.K, self.B = n, 1 << n, K, B
        self.o = Oracle(n, K, 0.32, crc, srand=1)
        C.CDLL(None).srand(C.c_uint(1))
        self.g = polar_amd.PolarCode(n, K, 0.32, crc)
        self.llr, self.info = self.o.synth_llr(seed, 0, B, self.o.snr_sqrt_linear(ebno))
        self.ordinary = _degenerate(self.llr, deg)
        assert 5 * len(deg) <= B or (B, tuple(deg)) == (B_CAP, DEG_CAP)        # (at most one row in five; the capped case: three of 14)
        self.llr.setflags(write=False)
        self._want, self._dev_rows = {}, {}

    def want(self, L):
        if L not in self._want:
            self._want[L] = self.o.decode_scl_llr(self.llr, L)
            self._want[L].setflags(write=False)
        return self._want[L]

    def dev_rows(self, rows=None):
        import torch
        a = self.llr if rows is None else rows
        if id(a) not in self._dev_rows:
            self._dev_rows[id(a)] = (a, torch.from_numpy(np.array(a)).cuda())
        return self._dev_rows[id(a)][1]


_cases = {}


def _capped(n, K, crc):
    if (n, K, crc) not in _cases:
        _cases[(n, K, crc)] = _Case(n, K, crc, B_CAP, 1.5, 4100 + n, DEG_CAP)
    return _cases[(n, K, crc)]


def _host(c, L, rows=None):
    return c.g.decode_scl_llr(c.llr if rows is None else rows, L)


def _dev(c, L, rows=None, B=None, with_pm=False):
    """The device-pointer entry point (collect and fallback in stream): (bits, path metrics as 64-bit patterns or None)."""
    import torch
    t = c.dev_rows(rows)
    B = t.shape[0] if B is None else B
    out = torch.zeros((B, c.K), dtype=torch.uint8, device="cuda")
    pm = torch.zeros(B, dtype=torch.float64, device="cuda") if with_pm else None
    pm_ptr = pm.data_ptr() if with_pm else 0
    if t.dtype == torch.float64:
        c.g.decode_scl_llr_dev(t.data_ptr(), B, L, out.data_ptr(), pm_ptr)
    else:
        c.g.decode_scl_llr_dev_fmt(t.data_ptr(), {torch.float32: "f32", torch.float16: "f16"}[t.dtype], B, L, out.data_ptr(), pm_ptr)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (pm.cpu().numpy().view(np.uint64) if with_pm else None)


def _both(g, decode, B, grid=0, trips=2, taken=True, slack=0):
    """golden_util.both_kernels (the batch kernel, then the latency form forced; asserts that they return the same on EVERY row) under the
    "lat_grid" cap, with the statement of what ran: the batch call took no latency kernel; the forced one did, with fewer blocks than
    rows and at least `trips` rows per block (+ slack rows) — or, taken=False, could not (the host's silent fall-back). Returns (result, blocks)."""
    waves = []

    def run():
        r = decode()
        waves.append(g.debug_get("lat_waves"))
        return r
    g.debug_set("lat_grid", grid)
    try:
        got = both_kernels(g, run)
    finally:
        g.debug_set("lat_grid", 0)
        g.debug_set("lat_max_b", 0)
    assert waves[0] == 0, f"lat_max_b = -1 took a latency kernel of {waves[0]} blocks"
    if taken:
        assert waves[1] > 0, "the forced call did not take the latency kernel"
        assert B > waves[1] and B >= trips * waves[1] + slack, (B, waves[1], trips)
        assert not grid or waves[1] == grid, (waves[1], grid)
    else:
        assert waves[1] == 0, f"a latency kernel of {waves[1]} blocks where none fits"
    return got, waves[1]


def _check_bits(c, L, taken, rows=None, want=None):
    """Both entry points: the host-pointer one (the deferred two-phase path with the flag read-back) and the device-pointer one."""
    want = c.want(L) if want is None else want
    for entry in (_host, lambda c_, L_, r_: _dev(c_, L_, r_)[0]):
        got, _ = _both(c.g, lambda: entry(c, L, rows), c.B, GRID, trips=4, taken=taken)
        bad = np.nonzero((got != want).any(axis=1) & c.ordinary)[0]
        assert bad.size == 0, f"ordinary rows {bad.tolist()} differ from the oracle"


# ---- (a) capped grid, many shapes ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", list(range(1, 9)))
@pytest.mark.parametrize("n,K,crc", CODES)
def test_capped_grid_every_list_size(built_lib, oracle_built, n, K, crc, L):
    """Three waves decode 14 rows, four or five each, at every list size 1 ... 8 (3, 5, 6 and 7 run a group wider than the list):
    list size 1 is sc_lat_kernel, 2 ... 8 the exp-domain latency form of the list kernel in groups of 2 / 4 / 8 lanes. At N = 4096
    the groups of 4 and 8 do not fit the LDS: there the forced call must fall back, and say so."""
    _check_bits(_capped(n, K, crc), L, taken=(n < 12 or L <= 2))


@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("n,K,crc", CODES)
def test_capped_grid_llr_domain_arithmetic(built_lib, oracle_built, n, K, crc, L):
    """Mode 1: groups of 2 lanes are the LLR-domain latency instantiation (it flags nothing: no fallback pass); a list of 4 has
    no latency form in this mode."""
    c = _capped(n, K, crc)
    c.g.set_mode(1)
    try:
        _check_bits(c, L, taken=(L == 2))
    finally:
        c.g.set_mode(0)


PM_CASES = [(n, K, crc, mode, L) for (n, K, crc) in CODES for (mode, L) in [(0, l) for l in range(2, 9)] + [(1, 2)]
            if n < 12 or L == 2]


@pytest.mark.parametrize("n,K,crc,mode,L", PM_CASES)
def test_capped_grid_path_metrics(built_lib, oracle_built, n, K, crc, mode, L):
    """The winning path's metric of every row, degenerate ones included, as the batch kernel returns it: the same 64 bits.

    Groups of 2 lanes in mode 0 are the case that needed a rule of its own: their batch kernel is the LLR-domain one, while the latency
    form runs the exp-domain nodes, whose leaf terms are -log(E) instead of |llr| — 3 ... 7 of these 14 metrics came out one ulp
    apart (2.0e-16 ... 3.9e-16 relative), capped or not. A call that asks for the metric now takes the LLR-domain latency form there
    (decode_list_lat), so that a row's metric does not depend on how many rows came with it."""
    c = _capped(n, K, crc)
    c.g.set_mode(mode)
    try:
        _both(c.g, lambda: _dev(c, L, with_pm=True)[1], c.B, GRID, trips=4)
    finally:
        c.g.set_mode(0)


def test_capped_grid_float_rows(built_lib, oracle_built):
    """float32 rows at (9, 300, 8), list of 4: widened in the latency kernel's own channel loads."""
    c = _capped(9, 300, 8)
    f = c.llr.astype(np.float32)
    _check_bits(c, 4, True, rows=f, want=c.o.decode_scl_llr(f.astype(np.float64), 4))


def test_capped_grid_half_rows(built_lib, oracle_built):
    """binary16 rows at (10, 512, 0), list size 1 (sc_lat_kernel reads the 16-bit rows in place)."""
    c = _capped(10, 512, 0)
    h = c.llr.astype(np.float16)
    _check_bits(c, 1, True, rows=h, want=c.o.decode_scl_llr(llr16_util.widen_f16(h), 1))


# ---- (b) the MLC receiver and decode_sc_p1 under the cap -------------------------------------------------------------------

@pytest.mark.parametrize("N", [256, 1024])
@pytest.mark.parametrize("const", ["ask4-sp", "ask16-sp", "ask16-gray"])
def test_capped_grid_mlc(built_lib, const, N):
    """mlc_sc_lat_kernel carries the re-encoded lower levels and the decisions from row to row. At the design SNR and 1 dB below,
    where lower levels decide wrongly: a wrong lower level left over from the previous row would change this one."""
    import polar_amd
    import torch
    import mlc_numpy as R
    from test_gpu_mlc import CASES, DESIGN, _handle
    K = N // 2
    src = [s for (c_, n_, s) in CASES if (c_, n_) == (const, N)]
    g, frozen, order = _handle(polar_amd, N, K, src[0] if src else None)
    cid = R.NAMES[const]
    for snr in (DESIGN[const], DESIGN[const] - 1.0):
        y, info = R.synth(frozen, order, K, cid, 5, np.arange(1000, 1000 + B_CAP, dtype=np.uint64), snr)
        _, n0 = R.sigma_n0(snr)
        want = R.decode(frozen, order, K, y, n0, cid)
        d_y = torch.from_numpy(y).cuda()

        def dev():
            out = torch.zeros((B_CAP, K), dtype=torch.float64, device="cuda")
            g.decode_mlc_dev(const, d_y.data_ptr(), n0, B_CAP, out.data_ptr())
            torch.cuda.synchronize()
            return out.cpu().numpy()
        for decode in (lambda: g.decode_mlc(y, n0, const), dev):
            got, _ = _both(g, decode, B_CAP, GRID, trips=4)
            assert np.array_equal(got, want, equal_nan=True), (const, N, snr, p1_rows.rows_that_differ(got, want))
    g.close()


@pytest.mark.parametrize("n,K", [(6, 32), (11, 1024)])
def test_capped_grid_sc_p1(built_lib, oracle_built, n, K):
    """sc_p1_lat_kernel at N = 64 and N = 2048 (test_gpu_sc_p1.py has a wave's second codeword at N = 4096 only); the degenerate rows
    of p1_rows come first and again at row 7, among ordinary ones."""
    o, g = p1_rows.pair(n, K, 0)
    p1, _ = p1_rows.rows(o, B_CAP, 1.0, every=7)
    want = np.stack([o.decode_sc_p1(p1[i]) for i in range(B_CAP)])
    got, _ = _both(g, lambda: g.decode_sc_p1(p1), B_CAP, GRID, trips=4)
    bad = p1_rows.rows_that_differ(got, want)
    assert bad.size == 0, bad
    g.close()


# ---- (c) the real grid, once per kernel -------------------------------------------------------------------------------------

REAL = [(12, 2048, 0, 1, 2.0, 8), (10, 512, 0, 1, 2.0, 8), (11, 1024, 16, 2, 2.0, 8), (9, 300, 8, 4, 2.0, 8), (7, 40, 0, 8, 2.0, 8),
        (11, 1024, 16, 8, 1.0, 2)]          # (the last one: one wave per CU; at 2 dB the oracle decodes every row right, hence 1 dB)


def _real(n, K, crc, L, ebno, per_cu):
    """No cap: B = per_cu * CUs + 3 rows (both host formulas launch at most 4 waves per CU), so that every wave of the launch the
    product makes decodes a second row and three of them a third one. Degenerate rows among the first and the last ten."""
    key = (n, K, crc, L, ebno, per_cu)
    if key not in _cases:
        B = per_cu * _cus() + 3
        _cases[key] = _Case(n, K, crc, B, ebno, 4000, (1, 5, 9, B - 9, B - 5, B - 1))
    return _cases[key]


def _later_rows_are_hard(c, L, w):
    """The later trips are not rows any sign decision would get right: the oracle itself decodes 1 % of them wrongly."""
    assert c.B - 9 >= w                                                  # (degenerate rows below and at or above the grid size)
    late = c.ordinary & (np.arange(c.B) >= w)
    wrong = int(((c.want(L) != c.info).any(axis=1) & late).sum())
    print(f"n={c.n} K={c.K} L={L}: {c.B} rows, {w} waves, the oracle decodes {wrong} of {int(late.sum())} later rows wrongly")
    assert 100 * wrong >= int(late.sum()), (wrong, int(late.sum()))


@pytest.mark.parametrize("n,K,crc,L,ebno,per_cu", REAL)
def test_real_grid_second_and_third_rows(built_lib, oracle_built, n, K, crc, L, ebno, per_cu):
    """sc_lat_kernel at N = 4096 and N = 1024, the latency form of the list kernel in groups of 2, 4 and 8 lanes, at the grid the
    host really launches."""
    c = _real(n, K, crc, L, ebno, per_cu)
    want = c.want(L)
    got, w = _both(c.g, lambda: _dev(c, L)[0], c.B, trips=2, slack=3)
    bad = np.nonzero((got != want).any(axis=1) & c.ordinary)[0]
    assert bad.size == 0, f"ordinary rows {bad[:8].tolist()} of {c.B} differ from the oracle ({w} waves)"
    _later_rows_are_hard(c, L, w)


@pytest.mark.parametrize("n,K,crc,L,ebno,per_cu", [r for r in REAL if r[3] >= 2])
def test_real_grid_path_metrics(built_lib, oracle_built, n, K, crc, L, ebno, per_cu):
    """The same rows: every row's metric as the batch kernel returns it, the same 64 bits."""
    c = _real(n, K, crc, L, ebno, per_cu)
    _, w = _both(c.g, lambda: _dev(c, L, with_pm=True)[1], c.B, trips=2, slack=3)
    _later_rows_are_hard(c, L, w)


@pytest.mark.parametrize("const,per_cu", [("ask4-sp", 2), ("ask16-sp", 3)])
def test_real_grid_mlc(built_lib, const, per_cu):
    """N = 2048: the LDS holds 2 (4-ASK) and 3 (16-ASK) waves per CU; 1 dB below the design SNR."""
    import polar_amd
    import mlc_numpy as R
    from test_gpu_mlc import DESIGN, _handle
    N, K = 2048, 1024
    B = 2 * per_cu * _cus() + 3
    g, frozen, order = _handle(polar_amd, N, K, None)
    cid = R.NAMES[const]
    snr = DESIGN[const] - 1.0
    y, info = R.synth(frozen, order, K, cid, 5, np.arange(1000, 1000 + B, dtype=np.uint64), snr)
    _, n0 = R.sigma_n0(snr)
    want = R.decode(frozen, order, K, y, n0, cid)
    got, w = _both(g, lambda: g.decode_mlc(y, n0, const), B, trips=2, slack=3)
    assert np.array_equal(got, want, equal_nan=True), p1_rows.rows_that_differ(got, want)[:8]
    wrong = int((want[w:] != info[w:]).any(axis=1).sum())
    print(f"{const} N={N} {snr} dB: {B} rows, {w} waves, the restatement decodes {wrong} of {B - w} later rows wrongly")
    assert 100 * wrong >= B - w, (wrong, B - w)
    g.close()


# ---- (d) the default dispatch at its threshold -----------------------------------------------------------------------------

def test_default_dispatch_at_its_threshold(built_lib, oracle_built):
    """lat_max_b = 0, (9, 300, 8). List of 4: two rounds of resident waves take the latency form, one row more takes the batch
    kernel (decode_list_lat). List size 1: 2048 rows against 2049 (use_sc_lat). The oracle's bits on both sides."""
    c = _Case(9, 300, 8, max(8 * _cus() + 3, 2049), 2.0, 4000, ())
    c.g.debug_set("lat_max_b", 1 << 40)
    try:
        _dev(c, 4)
        r = c.g.debug_get("lat_waves")
    finally:
        c.g.debug_set("lat_max_b", 0)
    assert 0 < r and 2 * r + 1 <= c.B
    for L, B, taken in ((4, 2 * r, r), (4, 2 * r + 1, 0), (1, 2048, None), (1, 2049, 0)):
        got, _ = _dev(c, L, B=B)
        w = c.g.debug_get("lat_waves")
        assert (w == taken) if taken is not None else (0 < w < B), (L, B, w, taken)
        assert (got == c.want(L)[:B]).all(), (L, B)
    c.g.close()
