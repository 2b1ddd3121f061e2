"""The two-phase decode of the lists of 17 .. 32 (polar_amd/csrc/polar_head_plan.h): the 4-lane head up to the hand-over leaf, the
list of 32 from there. Every result is compared bit for bit with the CPU oracle AND with the same call in one phase ("no_head");
path metrics, where asked for, must be the same doubles. "head_min_b" = 1 lets the small batches of a test take the head,
set_tuning(16) the default geometry (the small batches of the large lists otherwise run the fat-wave form, which has no head).
Rows are drawn at 0 and 1 dB so that the forks inside the head go both ways."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (n, K, crc) -> hand-over leaf
TAKEN = {(11, 1024, 16): 432,      # live layers 128 and 32
         (11, 512, 16): 496,       # one path at the hand-over; 247 all-frozen leaves past the prefix block
         (10, 256, 8): 368,        # n = 10 object, table mode
         (9, 128, 8): 208}         # generic-N object, no table mode
NOT_TAKEN = ((10, 512, 16),        # window of 17 leaves
             (11, 1800, 16))       # no prefix pass
_cache = {}


def setup(code, B=100):
    """-> (oracle, handle, llr rows [B, N], oracle's bits at L = 32), once per code"""
    if code not in _cache:
        import polar_amd
        from oracle_lib import Oracle
        n, K, crc = code
        o = Oracle(n, K, 0.32, crc, srand=1)
        C.CDLL(None).srand(C.c_uint(1))
        g = polar_amd.PolarCode(n, K, 0.32, crc)
        g.set_tuning(waves_per_cu=16)
        g.debug_set("head_min_b", 1)
        llr = np.concatenate([o.synth_llr(4242, 0, B // 2, o.snr_sqrt_linear(0.0))[0], o.synth_llr(4242, B // 2, B - B // 2, o.snr_sqrt_linear(1.0))[0]])
        _cache[code] = (o, g, llr, o.decode_scl_llr(llr, 32))
    return _cache[code]


def decode(g, llr, L, no_head, want_phi):
    """-> (bits, metrics) of one device call; checks what the launcher reports about the hand-over"""
    import torch
    B = llr.shape[0]
    d_llr = torch.from_numpy(np.ascontiguousarray(llr)).cuda()
    out = torch.full((B, g.K), 7, dtype=torch.uint8, device="cuda")
    pm = torch.zeros(B, dtype=torch.float64, device="cuda")
    g.debug_set("no_head", 1 if no_head else 0)
    try:
        g.decode_scl_llr_dev(d_llr.data_ptr(), B, L, out.data_ptr(), pm_ptr=pm.data_ptr())
        torch.cuda.synchronize()
        assert g.debug_get("head_phi") == (0 if no_head else want_phi)
    finally:
        g.debug_set("no_head", 0)
    return out.cpu().numpy(), pm.cpu().numpy()


def both_ways(g, llr, L, want_phi, want_bits):
    bits, pm = decode(g, llr, L, False, want_phi)
    bits1, pm1 = decode(g, llr, L, True, want_phi)
    assert (bits == want_bits).all(), np.nonzero((bits != want_bits).any(axis=1))[0][:10]
    assert (bits1 == want_bits).all()
    assert (pm.view(np.uint64) == pm1.view(np.uint64)).all(), np.nonzero(pm != pm1)[0][:10]


@pytest.mark.parametrize("code", sorted(TAKEN), ids=lambda c: "-".join(str(v) for v in c))
def test_head_taken(built_lib, oracle_built, code):
    o, g, llr, want = setup(code)
    both_ways(g, llr, 32, TAKEN[code], want)
    assert len({tuple(r[:64]) for r in want}) > 1          # (the rows do decode to different words)


@pytest.mark.parametrize("code", NOT_TAKEN, ids=lambda c: "-".join(str(v) for v in c))
def test_head_not_taken(built_lib, oracle_built, code):
    o, g, llr, want = setup(code, B=18)
    both_ways(g, llr, 32, 0, want)


@pytest.mark.parametrize("L", (20, 17))
def test_list_sizes_below_the_group(built_lib, oracle_built, L):
    """A lane offset other than 28 and a stack that is not the group's width."""
    for code in ((11, 1024, 16), (9, 128, 8)):
        o, g, llr, _ = setup(code)
        both_ways(g, llr[:33], L, TAKEN[code], o.decode_scl_llr(llr[:33], L))


@pytest.mark.parametrize("B", (1, 2, 15, 16, 17, 33, 100))
def test_batch_sizes(built_lib, oracle_built, B):
    """Partial 16-codeword waves in the head, partial pairs in the list of 32 (rows from the END of the set: other rows per size)."""
    o, g, llr, want = setup((11, 1024, 16))
    both_ways(g, llr[100 - B:], 32, 432, want[100 - B:])


def test_monte_carlo_rows_alive(built_lib, oracle_built):
    """mc_batch: from the second Eb/N0 point on only the first *n_dev rows of the batch are alive."""
    o, g, _, _ = setup((9, 128, 8))
    ebno, Ls = [0.0, 1.0, 2.0], [32]
    en = np.ones((1, 3), np.uint8)
    e1, r1 = np.zeros((1, 3), np.uint64), np.zeros((1, 3), np.uint64)
    e2, r2 = np.zeros((1, 3), np.uint64), np.zeros((1, 3), np.uint64)
    o.mc_batch(9, 0, 300, 1, ebno, Ls, en, e1, r1)
    g.mc_batch(9, 0, 300, 1, ebno, Ls, en, e2, r2)
    assert g.debug_get("head_phi") == 208
    assert (e1 == e2).all() and (r1 == r2).all()
    assert 0 < e1[0, 1] < e1[0, 0] < 300                   # (the later points did decode fewer rows than the batch holds)


def test_flagged_rows_take_the_fallback_pass(built_lib, oracle_built):
    """Rows the input guard flags — an element below 1e-9, a non-finite one — come back equal to the oracle: the flag the prefix
    pass set survives both phases."""
    o, g, llr, want = setup((11, 1024, 16))
    bad = llr[:20].copy()
    bad[3, 77] = 1e-12
    bad[8, 1500] = -3e-10
    bad[11, 100] = np.inf
    bad[16, 2047] = -np.inf
    want_bad = want[:20].copy()
    for i in (3, 8, 11, 16):
        want_bad[i] = o.decode_scl_llr(bad[i], 32)
    both_ways(g, bad, 32, 432, want_bad)


def test_head_no_head_head_on_one_handle(built_lib, oracle_built):
    """Nothing is left behind in the scratch or in the record buffer: both forms in turn, a smaller batch in between."""
    o, g, llr, want = setup((11, 1024, 16))
    for no_head, rows in ((False, slice(0, 40)), (True, slice(0, 40)), (False, slice(40, 57)), (True, slice(3, 9)), (False, slice(0, 40))):
        bits, _ = decode(g, llr[rows], 32, no_head, 432)
        assert (bits == want[rows]).all()


# ---- explicit masks (from_tables): hand-overs no Bhattacharyya code above reaches. The first three unfrozen leaves are placed by
# hand — the best channels their ranges have —, the rest of the mask is a Bhattacharyya code's unfrozen set beyond them; no CRC.
#   name: (n, base K, the three early leaves, base leaves kept from, expected hand-over, what it exercises)
EXPLICIT = {
    "n10-at-quarter": (10, 512, (191, 255, 271), 272, 256, "hand-over AT N/4 with table mode: phase B runs the first table build itself"),
    "n11-at-quarter": (11, 1024, (383, 511, 527), 528, 512, "the same at N = 2048"),
    "n10-capped": (10, 512, (255, 383), 512, 496, "third unfrozen leaf beyond N/2: the hand-over is capped, 16 below N/2"),
    "n11-capped": (11, 1024, (511, 767), 1024, 1008, "the same at N = 2048"),
    "n10-inside-block": (10, 512, (159, 223, 247), 256, 240, "hand-over below Q = 256: phase A resumes inside the prefix block, phase B too"),
}


def explicit_setup(name, B=40):
    key = ("explicit", name)
    if key not in _cache:
        import polar_amd
        from oracle_lib import Oracle
        n, Kb, early, keep_from, _, _ = EXPLICIT[name]
        N = 1 << n
        base = Oracle(n, Kb, 0.32, 16).frozen()
        frozen = np.ones(N, np.uint8)
        frozen[keep_from:] = base[keep_from:]
        frozen[list(early)] = 0
        K = int((frozen == 0).sum())
        order = np.concatenate([np.nonzero(frozen == 0)[0], np.nonzero(frozen)[0]]).astype(np.uint16)
        o = Oracle(n, K, 0.32, 0, srand=1)
        o.set_tables(frozen, order)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")              # (hand-placed leaves: the weak-leaves warning is expected)
            g = polar_amd.PolarCode.from_tables(n, K, 0, frozen, order)
        g.set_tuning(waves_per_cu=16)
        g.debug_set("head_min_b", 1)
        llr = np.concatenate([o.synth_llr(99, 0, B // 2, o.snr_sqrt_linear(0.0))[0], o.synth_llr(99, B // 2, B - B // 2, o.snr_sqrt_linear(1.0))[0]])
        _cache[key] = (o, g, llr, o.decode_scl_llr(llr, 32))
    return _cache[key]


@pytest.mark.parametrize("name", sorted(EXPLICIT))
def test_explicit_masks(built_lib, oracle_built, name):
    o, g, llr, want = explicit_setup(name)
    both_ways(g, llr, 32, EXPLICIT[name][4], want)
    assert len({tuple(r[:64]) for r in want}) > 1
