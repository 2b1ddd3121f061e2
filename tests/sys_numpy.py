"""Systematic polar coding in plain numpy: the four definitions the library's tables and kernels are held to, evaluated
on bytes with no packing and no short cuts.

Notation: `order`, K, crc, K' = K + crc, A' = order[0 .. K'), mask = the indicator of A'; z = butterfly(u) in natural order (stages
u[a] ^= u[a + inc]), coded[i] = z[bitrev(i)]; H the CRC matrix [crc][K]; T x = mask & butterfly(x); syndrome(u)[r] =
(sum_j H[r][j] u[order[j]]) ^ u[order[K + r]].

1. T^-1 by rounds: u = x, then `depth` times u = x ^ u ^ T u; depth = the least t >= 1 after which every unit vector of A' is solved.
2. Parity positions: walk i = K' - 1 .. 0, p = order[i], D_p = T^-1 e_p, c_p = syndrome(D_p); p is accepted when c_p is linearly
   independent of the accepted columns; stop at crc of them. par_u = the accepted positions in acceptance order, msg_u = A' without
   them in the order of `order`, Q = the accepted columns, n_swapped = the accepted positions outside order[K .. K').
3. Precode m -> u_info: x0[msg_u] = m; u = T^-1 x0; zP = Q^-1 syndrome(u); u ^= sum_r zP[r] D_{par_u[r]}; u_info = u[order[0 .. K)].
4. Message recovery u_info -> m: butterfly(place(u_info), check bits recomputed)[msg_u].
"""
import numpy as np


def butterfly(u):
    """The n stages u[a] ^= u[a + inc], inc = 1, 2, .., N / 2, over the last axis."""
    u = np.array(u, np.uint8)
    N = u.shape[-1]
    inc = 1
    while inc < N:
        v = u.reshape(u.shape[:-1] + (N // (2 * inc), 2, inc))
        v[..., 0, :] ^= v[..., 1, :]
        inc *= 2
    return u


def bitrev(n):
    i = np.arange(1 << n)
    r = np.zeros_like(i)
    for k in range(n):
        r |= ((i >> k) & 1) << (n - 1 - k)
    return r


def gf2_inverse(Q):
    """The inverse of a square 0 / 1 matrix over GF(2) (Gauss-Jordan); raises if it is singular."""
    c = len(Q)
    a = np.concatenate([np.array(Q, np.uint8) & 1, np.eye(c, dtype=np.uint8)], axis=1)
    for col in range(c):
        piv = col + int(np.flatnonzero(a[col:, col])[0])
        a[[col, piv]] = a[[piv, col]]
        for r in range(c):
            if r != col and a[r, col]:
                a[r] ^= a[col]
    return a[:, c:]


class Sys:
    """The systematic tables of a code (n, K, crc, order [N], H [crc][K])."""

    def __init__(self, n, K, crc, order, H=None):
        self.n, self.N, self.K, self.crc, self.Kp = n, 1 << n, K, crc, K + crc
        self.order = np.asarray(order, np.int64)
        self.H = np.zeros((crc, K), np.uint8) if crc == 0 else (np.asarray(H, np.uint8).reshape(crc, K) & 1)
        self.A = self.order[:self.Kp]
        self.mask = np.zeros(self.N, np.uint8)
        self.mask[self.A] = 1
        self.bitrev = bitrev(n)
        self.depth = self._depth()
        self._parity()
        self.pos = self.bitrev[self.msg_u]          # coded-row indices of the message bits
        self.par = self.bitrev[self.par_u]          # ... and of the parity positions

    def T(self, x):
        return self.mask & butterfly(x)

    def _depth(self):
        X = np.zeros((self.Kp, self.N), np.uint8)
        X[np.arange(self.Kp), self.A] = 1
        u = X.copy()
        for t in range(1, self.n + 2):
            u = X ^ u ^ self.T(u)
            if (self.T(u) == X).all():
                return t
        raise AssertionError("T^-1 did not converge in n + 1 rounds")

    def t_inv(self, x):
        x = np.asarray(x, np.uint8)
        u = x.copy()
        for _ in range(self.depth):
            u = x ^ u ^ self.T(u)
        return u

    def syndrome(self, u):
        u = np.asarray(u, np.uint8)
        info = u[..., self.order[:self.K]].astype(np.int64)
        return ((info @ self.H.T.astype(np.int64)) & 1).astype(np.uint8) ^ u[..., self.order[self.K:self.Kp]]

    def _parity(self):
        acc, cols, D = [], [], []
        basis = []                                   # reduced rows (as integers) for the independence test
        for i in range(self.Kp - 1, -1, -1):
            if len(acc) == self.crc:
                break
            p = int(self.order[i])
            e = np.zeros(self.N, np.uint8)
            e[p] = 1
            d = self.t_inv(e)
            c = self.syndrome(d)
            v = int(sum(int(b) << r for r, b in enumerate(c)))
            for b in basis:
                v = min(v, v ^ b)
            if v:
                basis.append(v)
                acc.append(p)
                cols.append(c)
                D.append(d)
        assert len(acc) == self.crc, "the walk over A' did not find crc independent columns"
        self.par_u = np.array(acc, np.int64)
        keep = ~np.isin(self.A, self.par_u)
        self.msg_u = self.A[keep]
        self.Q = np.array(cols, np.uint8).reshape(self.crc, self.crc).T          # column r = c of par_u[r]
        self.Qinv = gf2_inverse(self.Q) if self.crc else np.zeros((0, 0), np.uint8)
        self.D = np.array(D, np.uint8).reshape(self.crc, self.N)
        self.n_swapped = int((~np.isin(self.par_u, self.order[self.K:self.Kp])).sum())

    def place(self, u_info):
        """u [.., N] with u[order[i]] = u_info[i] and the check bits the CRC matrix gives."""
        u_info = np.asarray(u_info, np.uint8)
        u = np.zeros(u_info.shape[:-1] + (self.N,), np.uint8)
        u[..., self.order[:self.K]] = u_info
        if self.crc:
            u[..., self.order[self.K:self.Kp]] = (u_info.astype(np.int64) @ self.H.T.astype(np.int64)) & 1
        return u

    def encode(self, u_info):
        """The plain encoder: coded[i] = butterfly(place(u_info))[bitrev(i)]."""
        return butterfly(self.place(u_info))[..., self.bitrev]

    def precode(self, m):
        m = np.asarray(m, np.uint8)
        x0 = np.zeros(m.shape[:-1] + (self.N,), np.uint8)
        x0[..., self.msg_u] = m
        u = self.t_inv(x0)
        if self.crc:
            zP = (self.syndrome(u).astype(np.int64) @ self.Qinv.T.astype(np.int64)) & 1
            u = u ^ ((zP @ self.D.astype(np.int64)) & 1).astype(np.uint8)
        return u[..., self.order[:self.K]]

    def encode_systematic(self, m):
        u_info = self.precode(m)
        return self.encode(u_info), u_info

    def message(self, u_info):
        return butterfly(self.place(u_info))[..., self.msg_u]


def random_order(n, seed):
    """A seeded random permutation of the 2^n positions: the first K' entries are a frozen set no construction produces."""
    return np.random.default_rng(seed).permutation(1 << n).astype(np.uint16)


def frozen_of(order, Kp):
    f = np.ones(len(order), np.uint8)
    f[np.asarray(order[:Kp], np.int64)] = 0
    return f


def mirror_of(g):
    """The tables of a library handle."""
    return Sys(g.n, g.K, g.crc_size, g.channel_order_descending, g.crc_matrix if g.crc_size else None)


def random_code(seed, n=7):
    """A library handle over a seeded random frozen set of N = 2^n, K' = N / 2, with (odd seeds) a seeded CRC matrix of 8 rows. Such a
    set has weak leaves: it is encoded and recovered on, never decoded."""
    import warnings
    import polar_amd
    order = random_order(n, seed)
    crc = 8 * (seed & 1)
    K = (1 << n) // 2 - crc
    H = np.random.default_rng(seed).integers(0, 2, (crc, K)).astype(np.uint8) if crc else None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", polar_amd.PolarWeakLeavesWarning)
        return polar_amd.PolarCode.from_tables(n, K, crc, frozen_of(order, K + crc), order, H)


def swapped_code():
    """The library handle of swapped_case()."""
    import polar_amd
    frozen = polar_amd.PolarCode(SWAP_N, SWAP_K + SWAP_CRC, 0.32, 0).frozen_bits
    order, H, seed = swapped_case(frozen)
    assert seed is not None, "no CRC matrix with n_swapped > 0 within %d seeds" % SWAP_SEEDS
    return polar_amd.PolarCode.from_tables(SWAP_N, SWAP_K, SWAP_CRC, frozen, order, H)


SWAP_N, SWAP_K, SWAP_CRC, SWAP_SEEDS = 6, 24, 8, 64


def swapped_case(frozen):
    """A code whose parity walk leaves order[K .. K'): `frozen` is the constructed (6, 32) mask, `order` its unfrozen leaves in INDEX
    order (then the frozen ones), so the check positions are the 8 strongest leaves — whose D vectors reach far into the info positions
    — and the CRC matrix is the first of SWAP_SEEDS seeded ones with n_swapped > 0. On a constructed order the check positions are the
    weakest unfrozen leaves, D_p is next to e_p, and no matrix swaps anything. Returns (order, H, seed); seed None: none found."""
    frozen = np.asarray(frozen, np.uint8)
    order = np.concatenate([np.flatnonzero(frozen == 0), np.flatnonzero(frozen)]).astype(np.uint16)
    for seed in range(SWAP_SEEDS):
        H = np.random.default_rng(1000 + seed).integers(0, 2, (SWAP_CRC, SWAP_K)).astype(np.uint8)
        if Sys(SWAP_N, SWAP_K, SWAP_CRC, order, H).n_swapped > 0:
            return order, H, seed
    return order, None, None
