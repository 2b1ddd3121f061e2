"""Plain numpy models of the front and the back of the Monte-Carlo path (polar_amd/csrc/polar_channel.hip): the encoder
(encode_in_lds, the oracle's orc_encode), the block-error count (count_errors_kernel) and the sweep rule of a round with its alive
lists (mc_round_launch / mc_count_compact_kernel, the oracle's orc_mc_batch_impl), replayed trial set by trial set on the oracle's
per-trial generator and decoder. Shared by tests/test_sweep_model.py (CPU) and the GPU tests of the same kernels; the sweep cases
both use are defined here, so that what the CPU test asserts about the inputs holds for what the GPU test runs."""
import functools

import numpy as np


def encode(order, crcm, n, info):
    """info [B][K] (0 / 1) -> coded [B][N]: u[order[:K]] = info, the check bits crcm @ info mod 2 at order[K : K + crc], the n XOR
    stages u[a] ^= u[a + 2^it], and the bit-reversed read-out coded[i] = u[bitrev_n(i)]."""
    info = np.atleast_2d(np.asarray(info, np.uint8))
    B, K = info.shape
    N = 1 << n
    order = np.asarray(order, np.int64)
    crcm = np.asarray(crcm, np.uint8).reshape(-1, K)
    crc = crcm.shape[0]
    u = np.zeros((B, N), np.uint8)
    u[:, order[:K]] = info
    if crc:
        u[:, order[K:K + crc]] = ((info.astype(np.int64) @ crcm.T.astype(np.int64)) % 2).astype(np.uint8)
    for it in range(n):
        inc = 1 << it
        v = u.reshape(B, N // (2 * inc), 2, inc)
        v[:, :, 0, :] ^= v[:, :, 1, :]
    i = np.arange(N)
    br = np.zeros(N, np.int64)
    for k in range(n):
        br |= ((i >> k) & 1) << (n - 1 - k)
    return u[:, br]


def count_errors(a, b):
    """(flags [B], count): a row is in error when any of its bytes differs (bytes, not bits: 2 against 0 differs)."""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    flags = (a != b).any(axis=1)
    return flags, int(flags.sum())


def trial_indices(t0, T, stride):
    """t0 + i * stride for i < T, in 64-bit unsigned arithmetic"""
    return np.uint64(t0) + np.arange(T, dtype=np.uint64) * np.uint64(stride)


def mc_reference(o, seed, t0, T, stride, axis, Ls, enabled, cid=0):
    """One round of the sweep on the oracle `o` (tests/oracle_lib.py): per list size the alive set starts as all T trials; per
    enabled point the alive trials are generated AT THAT POINT, decoded and compared with what was sent, and the failing ones are
    the next alive set (a trial that decoded at a lower point counts as run and is not simulated again). Returns a dict of
    [n_L][n_e] uint64 arrays err, bit_err (differing info bits summed over the simulated trials), run and last_bit (simulated
    trials whose info bit K - 1 differs), and `failing`: {(li, ie): sorted uint64 array of the trial indices that failed there}
    for every enabled cell."""
    axis = np.asarray(axis, np.float64)
    n_L, n_e = len(Ls), len(axis)
    enabled = np.asarray(enabled, np.uint8).reshape(n_L, n_e)
    res = {k: np.zeros((n_L, n_e), np.uint64) for k in ("err", "bit_err", "run", "last_bit")}
    res["failing"] = {}
    for li, L in enumerate(Ls):
        alive = trial_indices(t0, T, stride)
        for ie in range(n_e):
            if not enabled[li, ie]:
                continue
            res["run"][li, ie] = T
            if len(alive):
                llr, info = o.synth_llr_trials(seed, alive, o.snr_sqrt_linear(axis[ie]) if cid == 0 else axis[ie], cid)
                diff = o.decode_scl_llr(llr, int(L)) != info
            else:
                diff = np.zeros((0, o.K), bool)
            nd = diff.sum(axis=1)
            res["err"][li, ie] = int((nd > 0).sum())
            res["bit_err"][li, ie] = int(nd.sum())
            res["last_bit"][li, ie] = int(diff[:, o.K - 1].sum())
            alive = np.sort(alive[nd > 0])
            res["failing"][(li, ie)] = alive
    return res


def last_lists(ref, T, t0, stride, enabled):
    """What the two alive buffers hold after the round, as a set of two sorted arrays: of the last list size that has an enabled
    point, the failures of its last enabled point and what that point was given (the failures of the enabled point before it, or
    all T trials)."""
    enabled = np.asarray(enabled, np.uint8)
    li = max(i for i in range(enabled.shape[0]) if enabled[i].any())
    pts = [ie for ie in range(enabled.shape[1]) if enabled[li, ie]]
    given = ref["failing"][(li, pts[-2])] if len(pts) > 1 else np.sort(trial_indices(t0, T, stride))
    return given, ref["failing"][(li, pts[-1])]


def _mask(n_L, n_e, off=()):
    en = np.ones((n_L, n_e), np.uint8)
    for li, ie in off:
        if ie is None:
            en[li, :] = 0
        else:
            en[li, ie] = 0
    return en


# The sweep cases of tests/test_gpu_sweep_edges.py. code = (n, K, crc); call = the entry point: "ber" (mc_batch_ber), "plain"
# (mc_batch) or "bicm" (mc_batch_bicm with constellation cid); the axis is Eb/N0 in dB (SNR in dB for "bicm"). `has` names the
# conditions tests/test_sweep_model.py asserts on the model's answer: "empty" (a cell nobody fails, with an enabled point of the
# same list size after it), "full" (a cell all T trials fail), "last_bit" (a failing trial whose info bit K - 1 differs),
# "cross" (failing trials on both sides of a multiple of 2^32).
SWEEP_CASES = {
    # short K and N: K below 64 and just above it (a lane-loop tail of one); one point off in the middle of L = 1, every point of
    # L = 2 off, the first point of L = 8 off
    "short_k21": dict(code=(6, 21, 3), call="ber", seed=101, t0=7, T=150, stride=1, Ls=[1, 2, 8], axis=[-10.0, -1.0, 1.5, 12.0, 14.0],
                      enabled=_mask(3, 5, [(0, 2), (1, None), (2, 0)]), has=("empty", "full", "last_bit")),
    "short_k65": dict(code=(7, 65, 0), call="ber", seed=102, t0=7, T=150, stride=1, Ls=[1, 2, 8], axis=[-10.0, -1.0, 1.5, 12.0, 14.0],
                      enabled=_mask(3, 5, [(0, 2), (1, None), (2, 0)]), has=("empty", "full", "last_bit")),
    # trial indices t0 + 3 i that cross 2^32 at i = 17
    "cross_2_32": dict(code=(6, 21, 3), call="ber", seed=103, t0=2**32 - 50, T=120, stride=3, Ls=[1, 4], axis=[-10.0, -2.0, 0.0],
                       enabled=_mask(2, 3), has=("full", "last_bit", "cross")),
    # more alive trials than blocks of the compaction kernel: the second point reads 8292 list entries
    "compaction": dict(code=(5, 16, 0), call="plain", seed=204, t0=0, T=8192 + 100, stride=1, Ls=[1], axis=[-30.0, -2.0, 2.0],
                       enabled=_mask(1, 3), has=("full",)),
    # the ASK axis with a label tail (8-ASK on N = 128: 42 symbols + 2 positions; 16-ASK on N = 64: no tail, 16 symbols)
    "ask8_k65": dict(code=(7, 65, 0), call="bicm", cid=2, seed=105, t0=3, T=120, stride=1, Ls=[1, 8], axis=[-5.0, 6.0, 9.0, 30.0],
                     enabled=_mask(2, 4), has=()),
    "ask16_k21": dict(code=(6, 21, 3), call="bicm", cid=3, seed=106, t0=3, T=120, stride=1, Ls=[1, 8], axis=[-5.0, 8.0, 12.0, 32.0],
                      enabled=_mask(2, 4), has=()),
    # the headline family once: list of 32 with a device row count, few rows left at the last point
    "headline": dict(code=(11, 1024, 16), call="plain", seed=107, t0=0, T=64, stride=1, Ls=[32], axis=[0.75, 1.0, 1.5],
                     enabled=_mask(1, 3), has=()),
}
# the pipelined driver on an edge code: the axis holds the full-list and the empty-list ends (asserted on one round of the model)
PIPELINE_CASE = dict(code=(7, 65, 0), seed=108, Ls=[1, 8], axis=[-10.0, -1.0, 1.5, 12.0, 14.0],
                     settings=((20, 100, 600), (10**6, 150, 450)))        # (max_err, batch, max_runs)


# the codes (n, K, crc) of tests/test_gpu_front_edges.py: N below 64, K below 64, K around 64 and 128, wide CRCs on short K
FRONT_CODES = [(1, 1, 0), (1, 2, 0), (2, 3, 1), (5, 16, 0), (5, 31, 1), (6, 1, 0), (6, 40, 24), (7, 63, 0), (7, 64, 8), (7, 65, 0),
               (8, 127, 0), (8, 129, 3), (8, 200, 16)]
# ... and of its ASK tests: one 8-ASK symbol + a tail of 1; 21 symbols + 1; 42 symbols + 2; 85 symbols (more than 64) + 1
ASK_CODES = [(2, 2, 0), (6, 21, 3), (7, 65, 0), (8, 129, 3)]


def info_rows(K, B, seed):
    """B info rows: random ones, with all-zero, all-one and the one-hot rows at index 0 and K - 1 in front (as many as B holds)"""
    info = np.random.default_rng(seed).integers(0, 2, (B, K)).astype(np.uint8)
    edge = np.zeros((4, K), np.uint8)
    edge[1] = 1
    edge[2, 0] = 1
    edge[3, K - 1] = 1
    m = min(B - 1, 4)                          # (B = 1: the random row alone)
    info[:m] = edge[:m]
    return info


# more trials than the 1024 x 256 threads that initialise the alive list; compared with the oracle's own engine
INIT_CASE = dict(code=(2, 2, 0), seed=10, t0=2**32 - 1000, T=262144 + 5, Ls=[1], axis=[-6.0, 3.0])


def make_oracle(code):
    from oracle_lib import Oracle
    n, K, crc = code
    return Oracle(n, K, 0.32, crc, srand=1)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """mc_reference of SWEEP_CASES[name], computed once per process and shared by the tests that need it (read only)."""
    c = SWEEP_CASES[name]
    o = make_oracle(c["code"])
    return mc_reference(o, c["seed"], c["t0"], c["T"], c["stride"], c["axis"], c["Ls"], c["enabled"], c.get("cid", 0))
