"""Rate-matched designs and the recovered rows every decoder is compared on over them (DESIGN.md §8k "Checks"). Shared by
tests/test_rm_cases.py (CPU: the conditions the mirrors need hold on these rows), tests/test_gpu_rm_compose.py (`rate_recover`, then
the list output, the adaptive, SC-Flip, SCAN, exp-domain and systematic calls) and tests/test_gpu_grid_trips.py (the workload).

A recovered row is unlike the rows the decoders' own suites draw: exact +0.0 at every punctured position, exactly 1000.0 at every
known one, sums of two received values at repeated ones, and a frozen set whose forced leaves sit at the very end of the tree.

Codes: seven designs of tests/test_gpu_rm.py's table (rm_numpy.design at phi_dx = 1e-4, on the numpy phi tables of ga_numpy.py — the
GPU file asserts that the device's design has the same frozen set and order). Rows: trials 0 .. 47 of the rate-matched workload at
seed 11 and the code's list-of-8 Eb/N0 of that table: the oracle's info bits and encoder, the shim's noise, rm_numpy.recover.
"""
import tempfile
import warnings

import numpy as np

import ga_numpy as G
import rm_numpy as M
import scl_list_numpy as S

PHI_DX = 1e-4
SEED = 11
ROWS = 48
EPS = 0.32
# (n, K, crc, E, scheme, design Eb/N0) -> the Eb/N0 of tests/test_gpu_rm.py SHAPES[key][8] (tests/test_rm_cases.py holds them equal)
CODES = {
    (5, 8, 8, 24, "puncture", 2.0): 2.0,
    (5, 8, 8, 24, "shorten", 2.0): 1.75,
    (5, 8, 8, 33, "repeat", 2.0): 1.75,
    (7, 48, 8, 100, "puncture", 2.0): 1.25,
    (7, 48, 8, 100, "shorten", 2.0): 1.25,
    (7, 32, 8, 100, "nr", 2.0): 0.75,
    (7, 56, 8, 100, "nr", 2.0): 1.5,
}
KEYS = list(CODES)
LIST_LS = (4, 8)
ADAPTIVE = (1, 4, 32)
FLIP_T = (0, 4)
SCAN_ROWS = 32
# test_rm_cases.py::test_scan_tolerance measures, over these seven codes and four draws of the perturbation, the largest deviation of a
# finite soft output between the exact SCAN model and the perturbed one on the margin rows at 4 iterations: 4.8e-11 (the n = 7 NR code
# that punctures; the other n = 7 codes 0.9e-11 .. 1.6e-11, the n = 5 codes 1.1e-12 .. 7.6e-12). Ten times that is far below
# mask_cases.SCAN_TOL = 2e-7, so that constant is the tolerance here too and SCAN_MARGIN = 100 SCAN_TOL selects the rows.
SCAN_DEV_MEASURED = 4.8e-11

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def phi_tables():
    return _once("phi", lambda: (G.phi_fwd(), G.phi_inv(PHI_DX)))


def shim():
    """rm_numpy's C shim around include/polar_synth.h, built once per process in a directory of its own."""
    def make():
        d = tempfile.TemporaryDirectory(prefix="rm_shim_")
        return d, M.build_shim(d.name)
    return _once("shim", make)[1]


def name(key):
    return "n%d-K%d-E%d-%s" % (key[0], key[1], key[3], key[4])


class Case:
    """One design: what scl_list_numpy.Code, the oracle and PolarCode.from_gauss_approx_rm take. The CRC matrix is the one
    from_gauss_approx_rm draws for its default seed; the oracle carries it too."""

    def __init__(self, key):
        self.key, self.name = key, name(key)
        self.n, self.K, self.crc, self.E, self.scheme, self.design_ebno = key
        self.N, self.ebno = 1 << self.n, CODES[key]
        self.d = M.design(self.n, self.K, self.crc, self.E, self.scheme, self.design_ebno, *phi_tables())
        self.sel, self.known = self.d["sel"], self.d["known"]
        self.punctured = M.punctured(self.n, self.sel, self.known)
        self._crcm = np.random.default_rng(1).integers(0, 2, (self.crc, self.K)).astype(np.uint8)
        self._o = None

    def __repr__(self):
        return self.name

    def frozen(self):
        return self.d["frozen"]

    def order(self):
        return self.d["order"]

    def crc_matrix(self):
        return self._crcm

    def oracle(self):
        if self._o is None:
            from oracle_lib import Oracle
            self._o = Oracle(self.n, self.K, EPS, self.crc, srand=1)
            self._o.set_tables(self.d["frozen"], self.d["order"])
            self._o.set_crc_matrix(self._crcm)
        return self._o

    def handle(self):
        """The device handle of the same design; a weak-leaf warning is an error, and the tables are the mirror's."""
        import polar_amd
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            g = polar_amd.PolarCode.from_gauss_approx_rm(self.N, self.K, self.E, self.scheme, self.design_ebno, self.crc, phi_dx=PHI_DX)
        assert g.weak_leaves == 0
        assert (g.frozen_bits == self.d["frozen"]).all() and (g.channel_order_descending == self.d["order"]).all()
        assert (g.crc_matrix == self._crcm).all()
        sel, known, short = g.rate_match_info()
        assert (sel == self.sel).all() and (known == self.known).all() and short == 1000.0
        return g

    def workload(self, trials, ebno=None, encode=None):
        """(rx [T, E], info [T, K]) of the given trials: the oracle's info bits, its encoder (or `encode`: info [T, K] -> coded
        [T, N]), the shim's noise at the rate K / E."""
        o = self.oracle()
        trials = np.asarray(trials, np.uint64)
        s = M.snr_sqrt_linear_rm(self.K, self.E, self.ebno if ebno is None else ebno)
        info = o.synth_llr_trials(SEED, trials, s)[1]
        coded = np.stack([o.encode(i) for i in info]) if encode is None else encode(info)
        return shim()(SEED, trials, s, coded[:, self.sel]), info

    def rows(self):
        """(rx [48, E], llr [48, N] = rm_numpy.recover(rx), info [48, K]), read-only."""
        def make():
            rx, info = self.workload(np.arange(ROWS))
            llr = M.recover(rx, self.sel, self.known)
            for a in (rx, llr, info):
                a.setflags(write=False)
            return rx, llr, info
        return _once(("rows", self.key), make)


def case(key):
    return _once(("case", key), lambda: Case(key))


def code(key):
    return _once(("code", key), lambda: S.Code(case(key)))


# ---- kept sets --------------------------------------------------------------------------------------------------------------------
def list_rows(key, Ls):
    """scl_list's survivors of every row per list size of Ls (None where it raises TieError: the row is left out for every list
    size) -> ({L: [rows]}, kept indices)."""
    def make():
        c, llr = code(key), case(key).rows()[1]
        lists, ok = {L: [] for L in Ls}, np.ones(len(llr), bool)
        for i in range(len(llr)):
            for L in Ls:
                try:
                    lists[L].append(S.scl_list(c, llr[i], L))
                except S.TieError:
                    lists[L].append(None)
                    ok[i] = False
        return lists, np.flatnonzero(ok)
    return _once(("list", key, tuple(Ls)), make)


def adaptive_reference(key):
    """(kept indices, (info, pm, stage, crc_ok) of adaptive_numpy.adaptive on them) under ADAPTIVE; a row on which a stage it
    reaches raises TieError is left out."""
    def make():
        import adaptive_numpy as A
        c, llr = code(key), case(key).rows()[1]
        kept, parts = [], []
        for i in range(len(llr)):
            try:
                parts.append(A.adaptive(c, llr[i:i + 1], ADAPTIVE))
                kept.append(i)
            except S.TieError:
                pass
        return np.array(kept, np.int64), tuple(np.concatenate([p[k] for p in parts]) for k in range(4))
    return _once(("adaptive", key), make)


def flip_keep(key):
    """bool [48]: mask_cases.flip_rows' rule on pass 0 — among the t_eff(max FLIP_T) + 1 smallest unfrozen magnitudes no two closer
    than 10 MARGIN relative, the smallest at least 10 MARGIN."""
    def make():
        import flip_numpy as F
        c, llr = code(key), case(key).rows()[1]
        _, leaf = F.sc_pass(c, llr)
        m = np.sort(np.abs(leaf[:, c.frozen == 0]), axis=1)
        head = m[:, :F.t_eff(c, max(FLIP_T)) + 1]
        gap = (np.diff(head, axis=1) / np.maximum(head[:, 1:], 1e-300)).min(axis=1)
        return (gap >= 10 * F.MARGIN) & (m[:, 0] >= 10 * F.MARGIN)
    return _once(("flip", key), make)


def scan_keep(key, margin=None):
    """bool [48]: no unfrozen leaf of the exact model below `margin` (default mask_cases.SCAN_MARGIN) in any of 4 iterations."""
    def make():
        import mask_cases as MC
        import scan_numpy as N
        c, llr = code(key), case(key).rows()[1]
        return N.row_margins(c, N.decode(c, llr, max(N.ITERS), check=False)) >= (MC.SCAN_MARGIN if margin is None else margin)
    return _once(("scan", key, margin), make)


def measure_scan_dev(key, draws=(0, 1, 2, 3)):
    """mask_cases.measure_scan_tol's measurement on the margin rows of one code: the largest deviation of a finite info_llr / ext entry
    between the exact SCAN model and the model with perturbed exp / log results, at 4 iterations."""
    import scan_numpy as N
    c, llr = code(key), case(key).rows()[1][scan_keep(key)]
    worst = 0.0
    a = N.decode(c, llr, max(N.ITERS), check=False)
    for seed in draws:
        b = N.decode(c, llr, max(N.ITERS), check=False, f=N.perturbed(np.random.default_rng(seed)))
        for k in ("info_llr", "ext"):
            fin = np.isfinite(a[k])
            assert (np.isfinite(b[k]) == fin).all()
            if fin.any():
                worst = max(worst, float(np.abs(a[k][fin] - b[k][fin]).max()))
    return worst


class Guard:
    """guard_numpy's criteria on the 48 recovered rows, as mask_cases.Rows states them: flag_* = the model says the fast kernels hand
    the row to the fallback pass, near_* = the row is within the model's own spare of a criterion (left out of the SET comparison,
    never of the bits). list: input_guard, row_tiny, the first descent's window; l1: input_guard, the all-frozen sum above 690, the
    product below 1e-8 or an exact zero at the root of an all-unfrozen node."""

    def __init__(self, key):
        import guard_numpy as GN
        import mask_cases as MC
        c, llr = code(key), case(key).rows()[1]
        u, _ = MC.sc_pass(c, llr)
        self.prod, self.fsum, self.zero, self.win = MC.margins(c, llr, u)
        self.bad_in = np.array([GN.input_guard(r) for r in llr])
        self.tiny = np.array([GN.row_tiny(r) for r in llr])
        self.first = np.array([GN.first_descent(r).min() for r in llr])
        self.flag_l1 = self.bad_in | (self.fsum > 690.0) | (self.prod < 1e-8) | self.zero
        self.near_l1 = ~self.bad_in & ((self.win < MC.WINDOW) | (np.abs(self.fsum - 690.0) <= 10.0) |
                                       ((self.prod >= 1e-9) & (self.prod < MC.PROD_MIN)))
        self.flag_list = self.bad_in | self.tiny
        self.near_list = ~self.flag_list & ((self.first < MC.WINDOW) | (self.win < MC.WINDOW))


def guard(key):
    return _once(("guard", key), lambda: Guard(key))


def list_near(key, L):
    """bool [48]: rows the input criteria do not flag on which guard_numpy.list_margins' walk at list size L (with the table build's
    hypotheses at 32) evaluates an f-node within mask_cases.WINDOW of |x| = 40, meets a tie, or has a weak leaf within 1e-6 of one:
    the list kernels' window criterion could go either way there."""
    def make():
        import guard_numpy as GN
        import mask_cases as MC
        c, llr, gd = code(key), case(key).rows()[1], guard(key)
        near = np.zeros(len(llr), bool)
        for i in np.flatnonzero(~gd.flag_list):
            try:
                m = GN.list_margins(c, llr[i], L, tables=L == 32)
                near[i] = bool(m.near(MC.WINDOW)) or m.min_weak() < 1e-6
            except S.TieError:
                near[i] = True
        return near
    return _once(("near", key, L), make)
