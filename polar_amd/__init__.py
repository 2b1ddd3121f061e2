"""polar_amd — MI355X-native polar SC/SCL decoder: Python host mirror of the reference's
``PolarCode`` class surface (PolarC/PolarCode.h:19-34, PolarM/PolarCode.m:59-93,266-322,781-850)
over the C-ABI of include/polar_amd.h.

This module is plumbing only: every compute call goes through ``libpolar_amd.so`` (hand-written
HIP kernels for gfx950). There is NO CPU fallback: if the shared library is missing, or no HIP
device is usable, the calls raise.
"""
import ctypes as C
import os

import numpy as np

try:  # must precede loading libpolar_amd.so so both share ONE HIP runtime (see build.py)
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is plumbing; the library also works stand-alone
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("POLAR_AMD_LIB") or os.path.join(_HERE, "libpolar_amd.so")   # (override: A/B builds)

_dp = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)
_u16p = C.POINTER(C.c_uint16)
_u64p = C.POINTER(C.c_uint64)


ASK4_GRAY, ASK8_GRAY, ASK16_GRAY, BPSK = 1, 2, 3, 4   # include/polar_synth.h POLAR_CONST_*
ASK4_SP, ASK8_SP, ASK16_SP = 5, 6, 7
CONSTELLATION_NAMES = {"bpsk": BPSK, "ask4-gray": ASK4_GRAY, "ask8-gray": ASK8_GRAY, "ask16-gray": ASK16_GRAY,
                       "ask4-sp": ASK4_SP, "ask8-sp": ASK8_SP, "ask16-sp": ASK16_SP}   # Constellation.m:41-66
_NBITS = {BPSK: 1, ASK4_GRAY: 2, ASK4_SP: 2, ASK8_GRAY: 3, ASK8_SP: 3, ASK16_GRAY: 4, ASK16_SP: 4}   # polar_const_nbits
RX_MLC = 0x100                 # include/polar_amd.h POLAR_RX_MLC
RECEIVERS = ("bicm", "mlc")


LLR_F64, LLR_F32, LLR_F16, LLR_BF16 = 0, 1, 2, 3     # include/polar_amd.h POLAR_LLR_*
LLR_FORMATS = {"f64": LLR_F64, "f32": LLR_F32, "f16": LLR_F16, "bf16": LLR_BF16}
LS_RUN, LS_ERR, LS_MISS, LS_UNDET, LS_ML, LS_N = 0, 1, 2, 3, 4, 5     # include/polar_amd.h POLAR_LS_*: columns of the list statistics
AD_RUN, AD_ERR, AD_UNDET, AD_STAGE0 = 0, 1, 2, 3     # include/polar_amd.h POLAR_AD_*: columns of the adaptive statistics (+ one per stage)
AD_MAX_STAGES = 8
FL_RUN, FL_ERR, FL_UNDET, FL_FIRST, FL_FLIPPED, FL_DECODES, FL_N = 0, 1, 2, 3, 4, 5, 6     # include/polar_amd.h POLAR_FL_*: columns of the SC-Flip statistics
FLIP_MAX = 64
SN_RUN, SN_ERR, SN_UNDET, SN_ITERS, SN_N = 0, 1, 2, 3, 4     # include/polar_amd.h POLAR_SN_*: columns of the SCAN statistics
SCAN_MINSUM, SCAN_EARLY_STOP, SCAN_MAX_ITERS = 1, 2, 32      # include/polar_amd.h POLAR_SCAN_*
SY_RUN, SY_ERR, SY_BIT_MSG, SY_BIT_U, SY_N = 0, 1, 2, 3, 4   # include/polar_amd.h POLAR_SY_*: columns of the systematic statistics
RM_PUNCTURE, RM_SHORTEN, RM_REPEAT, RM_NR = 0, 1, 2, 3       # include/polar_amd.h POLAR_RM_*: the built-in rate-matching schemes
RM_SCHEMES = {"puncture": RM_PUNCTURE, "shorten": RM_SHORTEN, "repeat": RM_REPEAT, "nr": RM_NR}
RM_RUN, RM_ERR, RM_BIT, RM_N = 0, 1, 2, 3                    # ... and the columns of the rate-matched statistics


def _llr_fmt_code(fmt):
    if isinstance(fmt, str):
        if fmt not in LLR_FORMATS:
            raise PolarError(f"unknown LLR format {fmt!r} (supported: {sorted(LLR_FORMATS)})")
        return LLR_FORMATS[fmt]
    return int(fmt)


def _llr_rows(llr, fmt):
    """(POLAR_LLR_* code, C-contiguous array) of the LLR rows of decode_scl_llr / decode_scl_llr_list: float32 and float16 arrays
    travel as they are, fmt="bf16" / "f16" take 16-bit patterns as uint16, anything else is taken as float64."""
    if fmt is not None:
        code = _llr_fmt_code(fmt)
        if code >= LLR_F16:
            ok = (np.uint16, np.float16) if code == LLR_F16 else (np.uint16,)
            if not (isinstance(llr, np.ndarray) and llr.dtype in ok):
                raise PolarError("fmt=%r takes the 16-bit patterns as a uint16 array%s" %
                                 (fmt, " (or the values as float16)" if code == LLR_F16 else ""))
            a = np.ascontiguousarray(llr)
        else:
            a = np.ascontiguousarray(llr, np.float32 if code == LLR_F32 else np.float64)
    elif isinstance(llr, np.ndarray) and llr.dtype == np.float32:
        code, a = LLR_F32, np.ascontiguousarray(llr)
    elif isinstance(llr, np.ndarray) and llr.dtype == np.float16:
        code, a = LLR_F16, np.ascontiguousarray(llr)
    else:
        code, a = LLR_F64, np.ascontiguousarray(llr, np.float64)
    return code, a


def _scan_flags(minsum, early_stop):
    return (SCAN_MINSUM if minsum else 0) | (SCAN_EARLY_STOP if early_stop else 0)


def _rx_flag(receiver):
    if receiver not in RECEIVERS:
        raise PolarError(f"unknown receiver {receiver!r} (supported: {RECEIVERS})")
    return RX_MLC if receiver == "mlc" else 0


def _constellation_id(c):
    if isinstance(c, str):
        if c not in CONSTELLATION_NAMES:
            raise PolarError(f"unsupported constellation {c!r} (supported: {sorted(CONSTELLATION_NAMES)})")
        return CONSTELLATION_NAMES[c]
    return int(c)


class PolarError(RuntimeError):
    pass


class PolarWeakLeavesWarning(UserWarning):
    """polar_create_explicit returned POLAR_W_WEAK_LEAVES (include/polar_amd.h)."""


POLAR_W_WEAK_LEAVES = 1


_lib = None


def lib():
    """Load libpolar_amd.so (built by polar_amd.build.build()); raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PolarError(
                f"{LIB_PATH} not found: build it with `python -m polar_amd.build` "
                "(the HIP extension is mandatory; there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        L.polar_last_error.restype = C.c_char_p
        L.polar_snr_sqrt_linear.restype = C.c_double
        L.polar_snr_sqrt_linear.argtypes = [C.c_void_p, C.c_double]
        if hasattr(L, "polar_snr_sqrt_linear_rm"):       # (POLAR_AMD_LIB may name an older build: A/B runs of the benchmark)
            L.polar_snr_sqrt_linear_rm.restype = C.c_double
            L.polar_snr_sqrt_linear_rm.argtypes = [C.c_void_p, C.c_double]
        _lib = L
    return _lib


def use_library(path=None):
    """Load another build of the library for everything created from now on (None = the product again). Handles belong to the
    library that made them: the caller keeps none across the switch. The tests of the failure protocol load the test build
    (libpolar_amd_test.so: the fault-injection hooks of include/polar_amd_debug.h exist only there)."""
    global _lib, LIB_PATH
    LIB_PATH = path or os.environ.get("POLAR_AMD_LIB") or os.path.join(_HERE, "libpolar_amd.so")
    _lib = None
    return lib()


def _check(rc):
    """Negative = error; positive = a non-error status (POLAR_W_WEAK_LEAVES), returned to the caller."""
    if rc < 0:
        raise PolarError(f"polar_amd error {rc}: {lib().polar_last_error().decode()}")
    return rc


def _p(a, t):
    return a.ctypes.data_as(t)


def _stream_ptr(stream):
    if stream is None:
        if torch is not None and torch.cuda.is_available():
            return C.c_void_p(torch.cuda.current_stream().cuda_stream)
        return C.c_void_p(0)
    if hasattr(stream, "cuda_stream"):
        return C.c_void_p(stream.cuda_stream)
    return C.c_void_p(int(stream))


class Constellation:
    """The reference's ``Constellation`` (PolarM/Constellation.m) over the C-ABI: ``Constellation("ask16-gray")`` has ``name``,
    ``n_bits``, ``n_sym``, ``points`` (normalised to unit mean energy, in symbol-index order, :19-32, 80), ``modulate`` (:84-93,
    on the host) and ``compute_llr_bicm`` (:123-144, on the GPU: there is no CPU path)."""

    def __init__(self, name):
        self.id = _constellation_id(name)
        if self.id not in _NBITS:
            raise PolarError(f"unknown constellation {name!r} (supported: {sorted(CONSTELLATION_NAMES)})")
        self.name = name if isinstance(name, str) else {v: k for k, v in CONSTELLATION_NAMES.items()}[self.id]
        self.n_bits = _NBITS[self.id]
        self.n_sym = 1 << self.n_bits
        # symbol s is what the bits of s (LSB first) modulate to
        labels = ((np.arange(self.n_sym)[:, None] >> np.arange(self.n_bits)[None, :]) & 1).astype(np.uint8)
        self.points = self.modulate(labels.reshape(-1))

    def modulate(self, bits):
        """bits [N] or [B][N] (0 / 1) -> symbols [floor(N / n_bits)] or [B][...]: symbol index = sum 2^j * bit j, LSB first."""
        a = np.ascontiguousarray(bits, np.uint8)
        if a.ndim not in (1, 2) or a.shape[-1] < 1:
            raise PolarError(f"modulate: bits must be [N] or [B][N], got shape {a.shape}")
        single = a.ndim == 1
        a2 = a.reshape(1, -1) if single else a
        out = np.zeros((a2.shape[0], a2.shape[1] // self.n_bits), np.float64)
        _check(lib().polar_modulate(C.c_int(self.id), _p(a2, _u8p), C.c_int(a2.shape[1]), C.c_long(a2.shape[0]), _p(out, _dp)))
        return out[0] if single else out

    def compute_llr_bicm(self, y, n0, block_length=None):
        """Constellation.compute_llr_bicm: (p1, llr) in the reference's output order, interleaved (position i*n_bits + j =
        label bit j of symbol i). y is [M] or [B][M], float64 or float32 (widened exactly on the device). ``block_length`` N
        (default M * n_bits) pads every row to N positions, the tail with llr = 0 / p1 = 0.5 (main_MC_CC_Comparison.m:94)."""
        f32 = isinstance(y, np.ndarray) and y.dtype == np.float32
        a = np.ascontiguousarray(y) if f32 else np.ascontiguousarray(y, np.float64)
        if a.ndim not in (1, 2):
            raise PolarError(f"compute_llr_bicm: y must be [M] or [B][M], got shape {a.shape}")
        single = a.ndim == 1
        a2 = a.reshape(1, -1) if single else a
        B, M = a2.shape
        N = M * self.n_bits if block_length is None else int(block_length)
        if N < 1 or N // self.n_bits != M:
            raise PolarError(f"compute_llr_bicm: rows of {M} symbols do not make rows of {N} positions at {self.n_bits} bits per symbol")
        p1, llr = np.zeros((B, N)), np.zeros((B, N))
        f = lib().polar_demap_bicm_f32 if f32 else lib().polar_demap_bicm
        _check(f(C.c_int(self.id), _p(a2, C.POINTER(C.c_float) if f32 else _dp), C.c_int(N), C.c_long(B), C.c_double(n0),
                 _p(llr, _dp), _p(p1, _dp)))
        return (p1[0], llr[0]) if single else (p1, llr)

    def compute_llr_bicm_dev(self, y_ptr, block_length, B, n0, llr_ptr=0, p1_ptr=0, stream=None, f32=False):
        """Device-resident form: y [B][block_length // n_bits] (float64, or float32 with f32=True) -> llr and / or p1
        [B][block_length] doubles (a pointer of 0 leaves that output out); asynchronous on `stream`."""
        f = lib().polar_demap_bicm_dev_f32 if f32 else lib().polar_demap_bicm_dev
        _check(f(C.c_int(self.id), C.c_void_p(y_ptr), C.c_int(block_length), C.c_long(B), C.c_double(n0),
                 C.c_void_p(llr_ptr), C.c_void_p(p1_ptr), _stream_ptr(stream)))


class PolarCode:
    """Drop-in for the reference ``PolarCode``.

    ``PolarCode(num_layers, info_length, epsilon, crc_size)`` follows PolarC (PolarCode.h:19);
    ``PolarCode.from_block_length(block_length, info_length, design_epsilon, crc_size=0)`` follows
    PolarM's argument order (PolarCode.m:59). ``PolarCode.from_tables`` takes explicit tables.
    """

    def __init__(self, num_layers, info_length, epsilon, crc_size=0, _handle=None):
        L = self._L = lib()          # (a handle belongs to the library that made it: use_library() may switch the default later)
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            self._chk(L.polar_create(C.c_int(num_layers), C.c_int(info_length), C.c_double(epsilon),
                                  C.c_int(crc_size), C.byref(self._h)))
        n, N, K, crc = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._chk(L.polar_get_params(self._h, C.byref(n), C.byref(N), C.byref(K), C.byref(crc)))
        self.n, self.block_length, self.info_length, self.crc_size = n.value, N.value, K.value, crc.value
        self.N, self.K = self.block_length, self.info_length

    @property
    def weak_leaves(self):
        """Unfrozen leaves the handle classified as weak at creation (polar_get_weak_leaves)."""
        return int(self._L.polar_get_weak_leaves(self._h))

    def debug_set(self, key, value):
        """Measurement knobs / test hooks of include/polar_amd_debug.h (polar_debug_set)."""
        self._chk(self._L.polar_debug_set(self._h, key.encode(), C.c_long(int(value))))

    def debug_get(self, key):
        f = self._L.polar_debug_get
        f.restype = C.c_long
        return int(f(self._h, key.encode()))

    def debug_fallback_rows(self):
        """The rows that the last decode_scl_llr call on device pointers handed to its fallback pass (polar_debug_fallback_rows), as a
        sorted uint32 array; None if the call had no fallback pass. Synchronises the call's stream."""
        f = self._L.polar_debug_fallback_rows
        f.restype = C.c_long
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_long]
        n = int(f(self._h, None, 0))
        if n == -1:
            return None
        if n < 0:
            raise PolarError(f"polar_debug_fallback_rows: HIP status {-n - 1}")
        rows = np.zeros(max(n, 1), np.uint32)
        if int(f(self._h, _p(rows, C.POINTER(C.c_uint32)), n)) != n:
            raise PolarError("polar_debug_fallback_rows: the count changed between two reads")
        return np.sort(rows[:n])

    def debug_mc_alive(self):
        """The two alive lists as the handle's last mc_batch / mc_batch_ber / mc_batch_bicm round left them (polar_debug_mc_alive):
        a pair of sorted uint64 arrays of trial indices, in buffer order; None before the first round."""
        f = self._L.polar_debug_mc_alive
        f.restype = C.c_long
        f.argtypes = [C.c_void_p, C.c_int, _u64p, C.c_long]
        lists = []
        for which in (0, 1):
            n = int(f(self._h, which, None, 0))
            if n == -1:
                return None
            if n < 0:
                raise PolarError(f"polar_debug_mc_alive: HIP status {-n - 1}")
            a = np.zeros(max(n, 1), np.uint64)
            if int(f(self._h, which, _p(a, _u64p), n)) != n:
                raise PolarError("polar_debug_mc_alive: the count changed between two reads")
            lists.append(np.sort(a[:n]))
        return tuple(lists)

    def debug_ctl_words(self, marked=True):
        """The per-leaf control words as uploaded (polar_debug_ctl_words): the array with the rate-1 block field, or the plain one."""
        f = self._L.polar_debug_ctl_words
        f.restype = C.c_long
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_long, C.c_int]
        words = np.zeros(self.N, np.uint32)
        n = int(f(self._h, _p(words, C.POINTER(C.c_uint32)), self.N, 1 if marked else 0))
        if n != self.N:
            raise PolarError(f"polar_debug_ctl_words: {n}")
        return words

    @classmethod
    def from_block_length(cls, block_length, info_length, design_epsilon, crc_size=0):
        n = int(round(np.log2(block_length)))
        if (1 << n) != block_length:
            raise PolarError("block_length must be a power of two")
        return cls(n, info_length, design_epsilon, crc_size)

    @classmethod
    def from_tables(cls, num_layers, info_length, crc_size, frozen, order, crc_matrix=None):
        frozen = np.ascontiguousarray(frozen, np.uint8)
        order = np.ascontiguousarray(order, np.uint16)
        N = 1 << num_layers
        if frozen.shape != (N,) or order.shape != (N,):
            raise PolarError("frozen/order must have N entries")
        cm = None
        if crc_size:
            cm = np.ascontiguousarray(crc_matrix, np.uint8)
            if cm.shape != (crc_size, info_length):
                raise PolarError("crc_matrix must be crc x K")
        h = C.c_void_p()
        status = _check(lib().polar_create_explicit(C.c_int(num_layers), C.c_int(info_length), C.c_int(crc_size),
                                                    _p(frozen, _u8p), _p(order, _u16p),
                                                    _p(cm, _u8p) if cm is not None else None, C.byref(h)))
        code = cls(num_layers, info_length, float("nan"), crc_size, _handle=h)
        if status == POLAR_W_WEAK_LEAVES:      # a valid handle; bit-exactness with the reference is limited (polar_amd.h)
            import warnings
            warnings.warn(f"polar_amd: {lib().polar_last_error().decode()}", PolarWeakLeavesWarning, stacklevel=2)
        return code

    @classmethod
    def from_construction_file(cls, path, info_length, crc_size=0, crc_matrix=None):
        """Code from a PolarM Monte-Carlo construction file (PolarM/CodeConstructionData/*.txt: one
        per-channel error count per line, written at PolarCode.m:120-124). As PolarCode.m:126-135:
        stable ascending sort of the counts, the first K+crc positions are the unfrozen set and their
        order is the info-bit order."""
        return cls.from_counts(np.loadtxt(path).reshape(-1), info_length, crc_size, crc_matrix)

    @classmethod
    def from_counts(cls, counts, info_length, crc_size=0, crc_matrix=None):
        """Code from a per-channel error-count table (PolarCode.m:126-135): stable ascending sort,
        the first K+crc positions are the unfrozen set and their order is the info-bit order."""
        counts = np.asarray(counts).reshape(-1)
        N = counts.size
        n = int(round(np.log2(N)))
        if (1 << n) != N:
            raise PolarError("the count table must hold a power-of-two number of entries")
        order = np.argsort(counts, kind="stable").astype(np.uint16)
        frozen = np.ones(N, np.uint8)
        frozen[order[: info_length + crc_size]] = 0
        return cls.from_tables(n, info_length, crc_size, frozen, order, crc_matrix)

    @classmethod
    def from_monte_carlo(cls, block_length, info_length, design_snr_db, crc_size=0, num_runs=100000,
                         constellation_name="bpsk", receiver_algo="bicm", seed=1, crc_matrix=None, data_dir=None):
        """Code designed by PolarM's `monte_carlo_code_construction` (PolarCode.m:95-141): same argument
        meaning and defaults; the genie-aided SC runs on the GPU (mc_construction).
        With ``data_dir`` the table is read from / written to
        ``MC_block_length_<unique string>.txt`` exactly as the reference does (:111-124)."""
        _rx_flag(receiver_algo)
        path = None
        if data_dir is not None:
            path = os.path.join(data_dir, "MC_block_length_" + construction_unique_string(
                block_length, info_length + crc_size, design_snr_db, constellation_name, receiver_algo, num_runs) + ".txt")
        if path is not None and os.path.exists(path):
            counts = np.loadtxt(path).reshape(-1)
        else:
            n = int(round(np.log2(block_length)))
            if (1 << n) != block_length:
                raise PolarError("block_length must be a power of two")
            counts = mc_construction(n, design_snr_db, num_runs, constellation_name, seed=seed, receiver=receiver_algo)
            if path is not None:
                write_construction_file(path, counts)
        if crc_size and crc_matrix is None:      # PolarCode.m:83: crc_matrix = floor(2*rand(crc_size, info_length))
            crc_matrix = np.random.default_rng(seed).integers(0, 2, (crc_size, info_length)).astype(np.uint8)
        code = cls.from_counts(counts, info_length, crc_size, crc_matrix)
        code.construction_counts = np.asarray(counts)
        # PolarCode.m:136: bler_estimate = sum(channels(info_bits)) / num_runs
        code.bler_estimate = float(np.sort(np.asarray(counts, np.float64), kind="stable")[: info_length + crc_size].sum() / num_runs)
        return code

    def monte_carlo_code_construction(self, design_snr_db, num_runs=100000, constellation_name="bpsk",
                                      receiver_algo="bicm", seed=1, data_dir=None):
        """In-place redesign of this code, as the reference method of the same name
        (PolarCode.m:95-141): block length, K, crc size and the crc matrix are kept, the frozen set and
        info-bit order are replaced."""
        cm = self.crc_matrix if self.crc_size else None
        new = PolarCode.from_monte_carlo(self.block_length, self.info_length, design_snr_db, self.crc_size, num_runs,
                                         constellation_name, receiver_algo, seed, cm, data_dir)
        self.close()
        self._h, new._h = new._h, None
        self.construction_counts, self.bler_estimate = new.construction_counts, new.bler_estimate
        return self.bler_estimate

    @classmethod
    def from_gauss_approx(cls, block_length, info_length, design_snr_db, constellation_name="bpsk", receiver_algo="bicm",
                          crc_size=0, crc_matrix=None, phi_dx=1e-5, seed=1, capacity=None):
        """Code designed by PolarM's `ga_code_construction` (PolarCode.m:198-255) on the GPU (ga_construction): capacities,
        mean LLRs, Gaussian-approximation polarization per sub-block, stable descending sort; the first K+crc positions
        are unfrozen and the order (most reliable first) is the handle's info-bit order, as from_counts passes it. Sets
        ``bler_estimate`` (sum of qfunc(sqrt(c)/sqrt(2)) over the unfrozen channels) and ``channels``. ``capacity`` (one
        value per label bit) replaces the computed capacities, e.g. by the reference's cached ones."""
        n = int(round(np.log2(block_length)))
        if (1 << n) != block_length:
            raise PolarError("block_length must be a power of two")
        cap = None if capacity is None else np.asarray(capacity, np.float64).reshape(1, -1)
        ch, order, pre = ga_construction(n, [design_snr_db], constellation_name, receiver_algo, phi_dx, seed, cap)
        k = info_length + crc_size
        if not 0 < k <= block_length:
            raise PolarError("info_length + crc_size must lie in [1, block_length]")
        frozen = np.ones(block_length, np.uint8)
        frozen[order[0, :k]] = 0
        if crc_size and crc_matrix is None:      # PolarCode.m:83: crc_matrix = floor(2*rand(crc_size, info_length))
            crc_matrix = np.random.default_rng(seed).integers(0, 2, (crc_size, info_length)).astype(np.uint8)
        code = cls.from_tables(n, info_length, crc_size, frozen, order[0], crc_matrix)
        code.channels = ch[0]
        code.bler_estimate = float(pre[0, k - 1])
        return code

    def ga_code_construction(self, design_snr_db, constellation_name="bpsk", receiver_algo="bicm", phi_dx=1e-5, seed=1,
                             capacity=None):
        """In-place redesign of this code by the Gaussian approximation, as the reference method of the same name
        (PolarCode.m:198-255): block length, K, crc size and the crc matrix are kept. Returns the BLER estimate."""
        cm = self.crc_matrix if self.crc_size else None
        new = PolarCode.from_gauss_approx(self.block_length, self.info_length, design_snr_db, constellation_name,
                                          receiver_algo, self.crc_size, cm, phi_dx, seed, capacity)
        self.close()
        self._h, new._h = new._h, None
        self.channels, self.bler_estimate = new.channels, new.bler_estimate
        return self.bler_estimate

    def _chk(self, rc):
        if rc < 0:
            raise PolarError(f"polar_amd error {rc}: {self._L.polar_last_error().decode()}")
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self._L.polar_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- tables ------------------------------------------------------------------------
    @property
    def frozen_bits(self):
        a = np.zeros(self.N, np.uint8)
        self._chk(self._L.polar_get_frozen(self._h, _p(a, _u8p)))
        return a

    @property
    def channel_order_descending(self):
        a = np.zeros(self.N, np.uint16)
        self._chk(self._L.polar_get_order(self._h, _p(a, _u16p)))
        return a

    @property
    def bit_rev_order(self):
        a = np.zeros(self.N, np.uint16)
        self._chk(self._L.polar_get_bitrev(self._h, _p(a, _u16p)))
        return a

    @property
    def crc_matrix(self):
        a = np.zeros((self.crc_size, self.K), np.uint8)
        if self.crc_size:
            self._chk(self._L.polar_get_crc_matrix(self._h, _p(a, _u8p)))
        return a

    @crc_matrix.setter
    def crc_matrix(self, m):
        m = np.ascontiguousarray(m, np.uint8)
        if m.shape != (self.crc_size, self.K):
            raise PolarError("crc_matrix must be crc x K")
        if self.crc_size:
            self._chk(self._L.polar_set_crc_matrix(self._h, _p(m, _u8p)))

    def reserve(self, B, list_size):
        """Pre-size the device scratch for decodes of up to B codewords at this list size (polar_reserve)."""
        self._chk(self._L.polar_reserve(self._h, C.c_long(B), C.c_int(list_size)))

    def set_tuning(self, waves_per_cu=0, lds_log=0):
        self._chk(self._L.polar_set_tuning(self._h, C.c_int(waves_per_cu), C.c_int(lds_log)))

    def set_mode(self, mode=0):
        """Node arithmetic of decode_scl_llr: 0 automatic, 1 LLR-domain kernel, 2 exp-domain kernel (+ fallback pass)."""
        self._chk(self._L.polar_set_mode(self._h, C.c_int(mode)))

    def snr_sqrt_linear(self, ebno_db):
        return self._L.polar_snr_sqrt_linear(self._h, C.c_double(ebno_db))

    # ---- encode (PolarCode.cpp:60-91) ---------------------------------------------------
    def encode(self, info_bits):
        info = np.ascontiguousarray(info_bits, np.uint8)
        single = info.ndim == 1
        info2 = info.reshape(-1, self.K)
        out = np.zeros((info2.shape[0], self.N), np.uint8)
        self._chk(self._L.polar_encode_batch(self._h, _p(info2, _u8p), C.c_long(info2.shape[0]), _p(out, _u8p)))
        return out[0] if single else out


    # ---- systematic coding ------------------------------------------------
    def systematic_info(self):
        """(depth, n_swapped) of the systematic tables (polar_get_sys_info): the rounds T^-1 takes on this frozen set (1 for every
        constructed code) and how many parity positions lie outside order[K .. K + crc). Host tables only: no GPU is needed."""
        d, s = C.c_int(), C.c_int()
        self._chk(self._L.polar_get_sys_info(self._h, C.byref(d), C.byref(s)))
        return d.value, s.value

    def systematic_positions(self):
        """(pos [K], par [crc]) uint16 (polar_get_sys_positions): the coded-row indices that carry the message bits —
        encode_systematic(m)[0][..., pos] == m — and those of the parity positions. Host tables only."""
        pos, par = np.zeros(self.K, np.uint16), np.zeros(self.crc_size, np.uint16)
        self._chk(self._L.polar_get_sys_positions(self._h, _p(pos, _u16p), _p(par, _u16p)))
        return pos, par

    def encode_systematic(self, msg):
        """Systematic encoder (polar_encode_sys_batch): msg [..., K] -> (coded [..., N], u_info [..., K]); coded == encode(u_info)
        and coded[..., pos] == msg with pos of systematic_positions()."""
        m = np.ascontiguousarray(msg, np.uint8)
        if m.shape[-1:] != (self.K,):
            raise PolarError(f"encode_systematic: msg must be [..., {self.K}], got shape {m.shape}")
        m2 = m.reshape(-1, self.K)
        coded = np.zeros((m2.shape[0], self.N), np.uint8)
        u = np.zeros((m2.shape[0], self.K), np.uint8)
        self._chk(self._L.polar_encode_sys_batch(self._h, _p(m2, _u8p), C.c_long(m2.shape[0]), _p(coded, _u8p), _p(u, _u8p)))
        return coded.reshape(m.shape[:-1] + (self.N,)), u.reshape(m.shape)

    def systematic_message(self, u_info):
        """Message recovery (polar_sys_message_batch): u_info [..., K] — a decoder's output, a whole list [B, L, K] — -> msg [..., K]."""
        u = np.ascontiguousarray(u_info, np.uint8)
        if u.shape[-1:] != (self.K,):
            raise PolarError(f"systematic_message: u_info must be [..., {self.K}], got shape {u.shape}")
        u2 = u.reshape(-1, self.K)
        out = np.zeros_like(u2)
        self._chk(self._L.polar_sys_message_batch(self._h, _p(u2, _u8p), C.c_long(u2.shape[0]), _p(out, _u8p)))
        return out.reshape(u.shape)

    def encode_systematic_dev(self, msg_ptr, B, coded_ptr=0, u_info_ptr=0, stream=None):
        """Device-resident form (polar_encode_sys_batch_dev): msg uint8 [B, K] -> coded uint8 [B, N] and / or u_info uint8 [B, K]."""
        self._chk(self._L.polar_encode_sys_batch_dev(self._h, C.c_void_p(msg_ptr), C.c_long(B), C.c_void_p(coded_ptr),
                                                     C.c_void_p(u_info_ptr), _stream_ptr(stream)))

    def systematic_message_dev(self, u_info_ptr, R, msg_ptr, stream=None):
        """Device-resident form (polar_sys_message_batch_dev): u_info uint8 [R, K] -> msg uint8 [R, K]; msg_ptr == u_info_ptr is allowed."""
        self._chk(self._L.polar_sys_message_batch_dev(self._h, C.c_void_p(u_info_ptr), C.c_long(R), C.c_void_p(msg_ptr),
                                                      _stream_ptr(stream)))

    def systematic_soft(self, llr, ext, fmt=None):
        """Soft message outputs (polar_sys_soft_batch): msg_llr [B, K] = (widen(llr) + ext)[:, pos], llr [B, N] (or [N]) and `fmt` as
        decode_scan, ext float64 of the same shape."""
        code, a = _llr_rows(llr, fmt)
        a2 = a.reshape(-1, self.N)
        e = np.ascontiguousarray(ext, np.float64).reshape(-1, self.N)
        if e.shape != a2.shape:
            raise PolarError("systematic_soft: llr and ext must have the same shape")
        out = np.zeros((a2.shape[0], self.K), np.float64)
        self._chk(self._L.polar_sys_soft_batch(self._h, C.c_void_p(a2.ctypes.data), C.c_int(code), _p(e, _dp), C.c_long(a2.shape[0]),
                                               _p(out, _dp)))
        return out

    def systematic_soft_dev(self, llr_ptr, fmt, ext_ptr, B, msg_llr_ptr, stream=None):
        """Device-resident form (polar_sys_soft_batch_dev)."""
        self._chk(self._L.polar_sys_soft_batch_dev(self._h, C.c_void_p(llr_ptr), C.c_int(_llr_fmt_code(fmt)), C.c_void_p(ext_ptr),
                                                   C.c_long(B), C.c_void_p(msg_llr_ptr), _stream_ptr(stream)))

    def synth_sys_llr_dev(self, seed, trial0, B, s_or_snr, llr_ptr, msg_ptr=0, u_info_ptr=0, constellation=0, stream=None):
        """polar_synth_sys_llr_dev: synth_llr_dev (constellation 0: s_or_snr = snr_sqrt_linear(Eb/N0)) or synth_bicm_llr_dev (an ASK
        constellation: the SNR in dB) with the systematic codeword of the trial's info bits, over the same noise."""
        self._chk(self._L.polar_synth_sys_llr_dev(self._h, C.c_int(_constellation_id(constellation)), C.c_uint64(seed), C.c_uint64(trial0),
                                                  C.c_long(B), C.c_double(s_or_snr), C.c_void_p(llr_ptr), C.c_void_p(msg_ptr),
                                                  C.c_void_p(u_info_ptr), _stream_ptr(stream)))

    def mc_batch_sys(self, seed, t0, T, stride, axis, list_size_vec, enabled, stats, constellation=0):
        """polar_mc_batch_sys: the trials {t0 + i*stride : i < T} of the systematic workload of every enabled (L, point) ADD to stats,
        uint64 [len(L), len(axis), 4] = SY_RUN, SY_ERR, SY_BIT_MSG, SY_BIT_U."""
        Ls = np.ascontiguousarray(list_size_vec, np.uint8)
        self._mc_batch_cells(self._L.polar_mc_batch_sys, seed, t0, T, stride, axis, Ls, enabled, stats, constellation, SY_N, True)

    def systematic_stats(self, axis, list_size_vec, max_runs=1000, max_err=100, seed=0, batch=0, constellation=0):
        """The systematic code over a sweep: rounds of mc_batch_sys, sized and stopped like list_stats' (_stat_rounds). Returns a dict:
        `stats` uint64 [len(L), len(axis), 4] (SY_* columns), `bler` = ERR over RUN, and `ber_msg`, `ber_u` = the wrong message bits and
        the wrong u-domain info bits of the same decodes over K RUN, float64 [len(L), len(axis)]."""
        ax = np.ascontiguousarray(axis, np.float64)
        Ls = np.ascontiguousarray(list_size_vec, np.uint8)
        stats = np.zeros((len(Ls), len(ax), SY_N), np.uint64)
        self._stat_rounds("systematic_stats", lambda t0, T, enabled: self.mc_batch_sys(seed, t0, T, 1, ax, Ls, enabled, stats, constellation),
                          stats, SY_ERR, SY_RUN, max_runs, max_err, batch)
        run = np.maximum(stats[:, :, SY_RUN], 1).astype(np.float64)
        return {"stats": stats, "bler": stats[:, :, SY_ERR] / run, "ber_msg": stats[:, :, SY_BIT_MSG] / (run * self.K),
                "ber_u": stats[:, :, SY_BIT_U] / (run * self.K)}

    # ---- rate matching ----------------------------------------------------
    @classmethod
    def from_gauss_approx_rm(cls, block_length, info_length, E, scheme, design_ebno_db, crc_size=0, crc_matrix=None, phi_dx=1e-5,
                             seed=1):
        """Code of E transmitted bits on the mother code of `block_length`, designed by the Gaussian approximation for the pattern
        of `scheme` (rate_match_pattern): the start vector is 4 (K / E) 10^(Eb/N0 / 10) times the number of transmit positions
        per coded position — 0 at a punctured one —, 1e4 at a known one; the forced leaves (rate_match_forced) go to the end of the
        order; the first K + crc of it are unfrozen; the pattern is set on the handle. Sets ``bler_estimate`` and ``channels`` as
        from_gauss_approx does."""
        n = int(round(np.log2(block_length)))
        if (1 << n) != block_length:
            raise PolarError("block_length must be a power of two")
        k = info_length + crc_size
        if not 0 < k <= block_length:
            raise PolarError("info_length + crc_size must lie in [1, block_length]")
        sel, known = rate_match_pattern(n, E, scheme, k)
        forced = rate_match_forced(n, sel, known)
        if k > block_length - int(forced.sum()):
            raise PolarError("info_length + crc_size exceeds the %d leaves this pattern leaves free" % (block_length - int(forced.sum())))
        init = (4 * (info_length / E) * 10 ** (design_ebno_db / 10)) * np.bincount(sel, minlength=block_length).astype(np.float64)
        init[known != 0] = 1e4
        ch, order, pre = ga_construction_init(n, init[None, :], forced, phi_dx)
        frozen = np.ones(block_length, np.uint8)
        frozen[order[0, :k]] = 0
        if crc_size and crc_matrix is None:      # PolarCode.m:83: crc_matrix = floor(2*rand(crc_size, info_length))
            crc_matrix = np.random.default_rng(seed).integers(0, 2, (crc_size, info_length)).astype(np.uint8)
        code = cls.from_tables(n, info_length, crc_size, frozen, order[0], crc_matrix)
        code.set_rate_match(sel, known)
        code.channels = ch[0]
        code.bler_estimate = float(pre[0, k - 1])
        return code

    def set_rate_match(self, sel, known=None, short_llr=1000.0):
        """The handle's rate-matching pattern (polar_set_rate_match): sel uint16 [E], known uint8 [N] or None."""
        sel = np.ascontiguousarray(sel, np.uint16).reshape(-1)
        if sel.size == 0:
            raise PolarError("set_rate_match: sel is empty (clear_rate_match removes a pattern)")
        kn = None
        if known is not None:
            kn = np.ascontiguousarray(known, np.uint8)
            if kn.shape != (self.N,):
                raise PolarError("set_rate_match: known must have N entries")
        self._chk(self._L.polar_set_rate_match(self._h, _p(sel, _u16p), C.c_int(sel.size), _p(kn, _u8p) if kn is not None else None,
                                               C.c_double(short_llr)))

    def clear_rate_match(self):
        self._chk(self._L.polar_set_rate_match(self._h, None, C.c_int(0), None, C.c_double(0.0)))

    def rate_match_info(self):
        """(sel uint16 [E], known uint8 [N], short_llr) of the pattern set (polar_get_rate_match), or None."""
        E, s = C.c_int(), C.c_double()
        self._chk(self._L.polar_get_rate_match(self._h, C.byref(E), None, None, None))
        if E.value == 0:
            return None
        sel, known = np.zeros(E.value, np.uint16), np.zeros(self.N, np.uint8)
        self._chk(self._L.polar_get_rate_match(self._h, C.byref(E), _p(sel, _u16p), _p(known, _u8p), C.byref(s)))
        return sel, known, s.value

    def _rm_E(self):
        E = C.c_int()
        self._chk(self._L.polar_get_rate_match(self._h, C.byref(E), None, None, None))
        if E.value == 0:
            raise PolarError("no rate-matching pattern set (set_rate_match)")
        return E.value

    def rate_match(self, coded):
        """coded [..., N] -> tx [..., E] = coded[..., sel] (polar_rate_match_batch)."""
        E = self._rm_E()
        c = np.ascontiguousarray(coded, np.uint8)
        if c.ndim < 1 or c.shape[-1] != self.N:
            raise PolarError(f"rate_match: coded must be [..., {self.N}], got shape {c.shape}")
        c2 = c.reshape(-1, self.N)
        tx = np.zeros((c2.shape[0], E), np.uint8)
        self._chk(self._L.polar_rate_match_batch(self._h, _p(c2, _u8p), C.c_long(c2.shape[0]), _p(tx, _u8p)))
        return tx.reshape(c.shape[:-1] + (E,))

    def rate_recover(self, rx, fmt=None):
        """rx [B, E] (or [E]; `fmt` as decode_scl_llr) -> the mother code's LLR rows float64 [B, N] (polar_rate_recover_batch):
        short_llr at a known position, the sum of the received values of a position in transmit order, +0.0 at a punctured one."""
        E = self._rm_E()
        code, a = _llr_rows(rx, fmt)
        if a.ndim < 1 or a.shape[-1] != E:
            raise PolarError(f"rate_recover: rx must be [..., {E}], got shape {a.shape}")
        a2 = a.reshape(-1, E)
        out = np.zeros((a2.shape[0], self.N), np.float64)
        self._chk(self._L.polar_rate_recover_batch(self._h, C.c_void_p(a2.ctypes.data), C.c_int(code), C.c_long(a2.shape[0]), _p(out, _dp)))
        return out[0] if a.ndim == 1 else out

    def decode_scl_llr_rm(self, rx, list_size, out=None, fmt=None):
        """decode_scl_llr of the rate-matched rows rx [B, E] (or [E]): rate_recover, then the decoder, in one call
        (polar_decode_scl_llr_rm_batch). `out` and `fmt` as decode_scl_llr."""
        E = self._rm_E()
        code, a = _llr_rows(rx, fmt)
        if a.ndim < 1 or a.shape[-1] != E:
            raise PolarError(f"decode_scl_llr_rm: rx must be [..., {E}], got shape {a.shape}")
        a2 = a.reshape(-1, E)
        if out is None:
            out = np.zeros((a2.shape[0], self.K), np.uint8)
        elif out.dtype != np.uint8 or out.shape != (a2.shape[0], self.K) or not out.flags.c_contiguous:
            raise PolarError("out must be a C-contiguous uint8 array of shape [B, K]")
        self._chk(self._L.polar_decode_scl_llr_rm_batch(self._h, C.c_void_p(a2.ctypes.data), C.c_int(code), C.c_long(a2.shape[0]),
                                                        C.c_int(list_size), _p(out, _u8p)))
        return out[0] if a.ndim == 1 else out

    def rate_match_dev(self, coded_ptr, B, tx_ptr, stream=None):
        """Device-resident form (polar_rate_match_batch_dev): coded uint8 [B, N] -> tx uint8 [B, E]."""
        self._chk(self._L.polar_rate_match_batch_dev(self._h, C.c_void_p(coded_ptr), C.c_long(B), C.c_void_p(tx_ptr), _stream_ptr(stream)))

    def rate_recover_dev(self, rx_ptr, fmt, B, llr_ptr, stream=None):
        """Device-resident form (polar_rate_recover_batch_dev): rx [B, E] of `fmt` -> llr float64 [B, N]."""
        self._chk(self._L.polar_rate_recover_batch_dev(self._h, C.c_void_p(rx_ptr), C.c_int(_llr_fmt_code(fmt)), C.c_long(B),
                                                       C.c_void_p(llr_ptr), _stream_ptr(stream)))

    def decode_scl_llr_rm_dev(self, rx_ptr, fmt, B, list_size, out_ptr, pm_ptr=0, stream=None):
        """Device-resident form (polar_decode_scl_llr_rm_batch_dev): rx [B, E] of `fmt` -> out uint8 [B, K], pm float64 [B]."""
        self._chk(self._L.polar_decode_scl_llr_rm_batch_dev(self._h, C.c_void_p(rx_ptr), C.c_int(_llr_fmt_code(fmt)), C.c_long(B),
                                                            C.c_int(list_size), C.c_void_p(out_ptr), C.c_void_p(pm_ptr), _stream_ptr(stream)))

    def snr_sqrt_linear_rm(self, ebno_db):
        return self._L.polar_snr_sqrt_linear_rm(self._h, C.c_double(ebno_db))

    def synth_rm_llr_dev(self, seed, trial0, B, s, rx_ptr, info_ptr=0, stream=None):
        """polar_synth_rm_llr_dev: the rate-matched workload's trials trial0 .. trial0 + B - 1: rx float64 [B, E], info uint8 [B, K]."""
        self._chk(self._L.polar_synth_rm_llr_dev(self._h, C.c_uint64(seed), C.c_uint64(trial0), C.c_long(B), C.c_double(s),
                                                 C.c_void_p(rx_ptr), C.c_void_p(info_ptr), _stream_ptr(stream)))

    def mc_batch_rm(self, seed, t0, T, stride, ebno_vec, list_size_vec, enabled, stats):
        """polar_mc_batch_rm: the trials {t0 + i*stride : i < T} of the rate-matched workload of every enabled (L, Eb/N0) ADD to
        stats, uint64 [len(L), len(ebno), 3] = RM_RUN, RM_ERR, RM_BIT."""
        Ls = np.ascontiguousarray(list_size_vec, np.uint8)
        fn = lambda h, _cid, *rest: self._L.polar_mc_batch_rm(h, *rest)       # (the sweep has no constellation argument: BPSK)
        self._mc_batch_cells(fn, seed, t0, T, stride, ebno_vec, Ls, enabled, stats, 0, RM_N, True)

    def rm_stats(self, axis, list_size_vec, max_runs=1000, max_err=100, seed=0, batch=0):
        """The rate-matched code over an Eb/N0 sweep: rounds of mc_batch_rm, sized and stopped like list_stats' (_stat_rounds).
        Returns a dict: `stats` uint64 [len(L), len(axis), 3] (RM_* columns), `bler` = ERR / RUN, `ber` = BIT / (RUN K)."""
        ax = np.ascontiguousarray(axis, np.float64)
        Ls = np.ascontiguousarray(list_size_vec, np.uint8)
        stats = np.zeros((len(Ls), len(ax), RM_N), np.uint64)
        self._stat_rounds("rm_stats", lambda t0, T, enabled: self.mc_batch_rm(seed, t0, T, 1, ax, Ls, enabled, stats),
                          stats, RM_ERR, RM_RUN, max_runs, max_err, batch)
        run = np.maximum(stats[:, :, RM_RUN], 1).astype(np.float64)
        return {"stats": stats, "bler": stats[:, :, RM_ERR] / run, "ber": stats[:, :, RM_BIT] / (run * self.K)}

    # ---- decoders -----------------------------------------------------------------------
    def decode_scl_llr(self, llr, list_size, out=None, fmt=None, systematic=False):
        """PolarCode::decode_scl_llr (PolarCode.cpp:130-148). `llr` is [N] or [B, N]; float32 and float16 arrays travel as
        they are and are widened exactly on the device, anything else is taken as float64. fmt="bf16": `llr` holds bfloat16
        bit patterns as uint16 (numpy has no bfloat16); fmt="f16" takes binary16 patterns as uint16 likewise. The result is
        the float64 call's on the widened values, bit for bit.
        out (optional): a C-contiguous uint8 [B, K] array to receive the bits (a caller that decodes batch after batch keeps
        one: a fresh 64-MiB array costs its page faults on every call).
        systematic=True: the rows carry systematic codewords (encode_systematic); the decoded word goes through the message step
        (systematic_message, in place in `out`) and the MESSAGE bits are returned."""
        code, a = _llr_rows(llr, fmt)
        single = a.ndim == 1
        a2 = a.reshape(-1, self.N)
        if out is None:
            out = np.zeros((a2.shape[0], self.K), np.uint8)
        elif out.dtype != np.uint8 or out.shape != (a2.shape[0], self.K) or not out.flags.c_contiguous:
            raise PolarError("out must be a C-contiguous uint8 array of shape [B, K]")
        self._chk(self._L.polar_decode_scl_llr_batch_fmt(self._h, C.c_void_p(a2.ctypes.data), C.c_int(code), C.c_long(a2.shape[0]),
                                                    C.c_int(list_size), _p(out, _u8p)))
        if systematic:
            self._chk(self._L.polar_sys_message_batch(self._h, _p(out, _u8p), C.c_long(a2.shape[0]), _p(out, _u8p)))
        return out[0] if single else out

    def decode_scl_llr_list(self, llr, list_size, fmt=None):
        """Every path the list decoder holds at the end of each codeword (polar_decode_scl_llr_list_batch): returns
        (cand [B, L, K] uint8, pm [B, L] float64, crc_ok [B, L] uint8, n_active [B] int32, winner [B] int32). Rows are ordered
        CRC pass first, then by metric; rows >= n_active are padding (bits 0, pm = inf, crc_ok = 0); cand[b, winner[b]] is what
        decode_scl_llr returns (winner = -1: the all-zero word). `llr` and `fmt` as decode_scl_llr; a single row [N] is a batch
        of one. Any list size 1 .. 64."""
        code, a = _llr_rows(llr, fmt)
        a2 = a.reshape(-1, self.N)
        B, L = a2.shape[0], int(list_size)
        if not 1 <= L <= 64:
            raise PolarError("list size %d out of range [1, 64]" % L)
        cand = np.zeros((B, L, self.K), np.uint8)
        pm = np.zeros((B, L), np.float64)
        crc_ok = np.zeros((B, L), np.uint8)
        n_active = np.zeros(B, np.int32)
        winner = np.zeros(B, np.int32)
        self._chk(self._L.polar_decode_scl_llr_list_batch(
            self._h, C.c_void_p(a2.ctypes.data), C.c_int(code), C.c_long(B), C.c_int(L), C.c_void_p(cand.ctypes.data),
            C.c_void_p(pm.ctypes.data), C.c_void_p(crc_ok.ctypes.data), C.c_void_p(n_active.ctypes.data),
            C.c_void_p(winner.ctypes.data)))
        return cand, pm, crc_ok, n_active, winner

    def decode_scl_llr_list_dev(self, llr_ptr, fmt, B, list_size, cand_ptr, pm_ptr=0, crc_ok_ptr=0, n_active_ptr=0, winner_ptr=0,
                                stream=None):
        """Device-resident form (polar_decode_scl_llr_list_batch_dev): LLRs [B, N] of format `fmt` -> cand uint8 [B, L, K] and,
        where a pointer is given, pm float64 [B, L], crc_ok uint8 [B, L], n_active int32 [B], winner int32 [B]; asynchronous
        on `stream`."""
        self._chk(self._L.polar_decode_scl_llr_list_batch_dev(
            self._h, C.c_void_p(llr_ptr), C.c_int(_llr_fmt_code(fmt)), C.c_long(B), C.c_int(list_size), C.c_void_p(cand_ptr),
            C.c_void_p(pm_ptr), C.c_void_p(crc_ok_ptr), C.c_void_p(n_active_ptr), C.c_void_p(winner_ptr), _stream_ptr(stream)))

    def list_find_dev(self, cand_ptr, n_active_ptr, info_ptr, B, list_size, rank_ptr, stream=None):
        """rank int32 [B] = the first row < n_active[b] of cand [B, L, K] whose bits equal info [B, K], or L (polar_list_find_dev);
        device pointers, asynchronous on `stream`."""
        self._chk(self._L.polar_list_find_dev(self._h, C.c_void_p(cand_ptr), C.c_void_p(n_active_ptr), C.c_void_p(info_ptr),
                                              C.c_long(B), C.c_int(list_size), C.c_void_p(rank_ptr), _stream_ptr(stream)))

    def path_metric(self, llr, info, fmt=None):
        """The metric the list decoder assigns to given words (polar_path_metric_batch): `llr` [B, N] (or [N]) and `fmt` as
        decode_scl_llr_list, `info` uint8 [B, K] (one word per row) or [B, R, K] (R <= 64 words per row, sharing the row) ->
        float64 [B] or [B, R]. Check bits are the CRC matrix's, frozen bits 0. Where decode_scl_llr_list holds the word with
        crc_ok = 1 the value equals that row's pm bit for bit."""
        code, a = _llr_rows(llr, fmt)
        a2 = a.reshape(-1, self.N)
        B = a2.shape[0]
        w = np.ascontiguousarray(info, np.uint8)
        if w.ndim == 1 and B == 1:
            w = w.reshape(1, -1)
        if w.ndim not in (2, 3) or w.shape[0] != B or w.shape[-1] != self.K:
            raise PolarError(f"path_metric: info must be [B, K] or [B, R, K] with B = {B}, K = {self.K}, got shape {w.shape}")
        R = 1 if w.ndim == 2 else w.shape[1]
        if not 1 <= R <= 64:
            raise PolarError("path_metric: %d words per row out of range [1, 64]" % R)
        pm = np.zeros((B,) if w.ndim == 2 else (B, R), np.float64)
        self._chk(self._L.polar_path_metric_batch(self._h, C.c_void_p(a2.ctypes.data), C.c_int(code), C.c_void_p(w.ctypes.data),
                                                  C.c_long(B), C.c_int(R), C.c_void_p(pm.ctypes.data)))
        return pm

    def path_metric_dev(self, llr_ptr, fmt, info_ptr, B, R, pm_ptr, stream=None):
        """Device-resident form (polar_path_metric_batch_dev): LLRs [B, N] of format `fmt`, info uint8 [B, R, K] -> pm float64
        [B, R]; asynchronous on `stream`."""
        self._chk(self._L.polar_path_metric_batch_dev(self._h, C.c_void_p(llr_ptr), C.c_int(_llr_fmt_code(fmt)), C.c_void_p(info_ptr),
                                                      C.c_long(B), C.c_int(R), C.c_void_p(pm_ptr), _stream_ptr(stream)))

    def mc_batch_list(self, seed, t0, T, stride, axis, list_size_vec, enabled, stats, constellation=0):
        """polar_mc_batch_list: the trials {t0 + i*stride : i < T} of every enabled (L, point) ADD to stats, uint64
        [len(L), len(axis), 5] = LS_RUN, LS_ERR, LS_MISS, LS_UNDET, LS_ML. constellation 0: BPSK, `axis` = Eb/N0 in dB; an
        ASK constellation: the BICM front end, `axis` = SNR in dB."""
        Ls = np.ascontiguousarray(list_size_vec, np.uint8)
        self._mc_batch_cells(self._L.polar_mc_batch_list, seed, t0, T, stride, axis, Ls, enabled, stats, constellation, LS_N, True)

    def _mc_batch_cells(self, fn, seed, t0, T, stride, axis, Ls, enabled, stats, constellation, cols, per_L):
        """polar_mc_batch_list / _adaptive: `cols` counters and one `enabled` byte per cell (a point; per_L: times a list size)."""
        ax = np.ascontiguousarray(axis, np.float64)
        enabled = np.ascontiguousarray(enabled, np.uint8)
        cells, txt = (len(Ls) * len(ax), ("len(L)", "len(axis)")) if per_L else (len(ax), ("len(axis)",))
        if stats.dtype != np.uint64 or stats.size != cells * cols or not stats.flags.c_contiguous:
            raise PolarError("stats must be a C-contiguous uint64 array [%s, %d]" % (", ".join(txt), cols))
        if enabled.size != cells:
            raise PolarError("enabled must have %s entries" % " * ".join(txt))
        self._chk(fn(self._h, C.c_int(_constellation_id(constellation)), C.c_uint64(seed), C.c_uint64(t0), C.c_long(T), C.c_long(stride),
                     _p(ax, _dp), C.c_int(len(ax)), _p(Ls, _u8p), C.c_int(len(Ls)), _p(enabled, _u8p), _p(stats, _u64p)))

    @staticmethod
    def _stat_rounds(who, batch_fn, stats, err_col, run_col, max_runs, max_err, batch):
        """The rounds list_stats and adaptive_stats share: batch_fn(t0, T, enabled) ADDS the trials t0 .. t0 + T - 1 of the enabled
        cells to `stats` ([..., columns]). `batch` trials a round; 0: max(256, 2 max_err) first, then doubling up to 262144. A cell
        leaves once ERR > max_err or RUN >= max_runs; no round goes past max_runs; the rounds end when no cell is left."""
        if max_runs < 1 or batch < 0:
            raise PolarError(who + ": max_runs must be positive and batch non-negative")
        done, step = 0, int(batch) if batch else max(256, 2 * int(max_err))
        while done < max_runs:
            enabled = ((stats[..., err_col] <= max_err) & (stats[..., run_col] < max_runs)).astype(np.uint8)
            if not enabled.any():
                break
            T = min(step, max_runs - done)
            batch_fn(done, T, enabled)
            done += T
            if not batch:
                step = min(2 * step, 262144)

    def list_stats(self, axis, list_size_vec, max_runs=1000, max_err=100, seed=0, batch=0, constellation=0):
        """Error analysis of the list decoder over a sweep: rounds of mc_batch_list (`batch` trials each; 0: max(256, 2 max_err)
        first, then doubling up to 262144), a point leaves the sweep once ERR > max_err or RUN >= max_runs (no round takes a point
        past max_runs). Returns a dict: `stats` uint64 [len(L), len(axis), 5] (LS_* columns), and `bler`, `miss_rate`,
        `undetected_rate`, `ml_bound` = ERR, MISS, UNDET, ML over RUN, float64 [len(L), len(axis)]."""
        ax = np.ascontiguousarray(axis, np.float64)
        Ls = np.ascontiguousarray(list_size_vec, np.uint8)
        stats = np.zeros((len(Ls), len(ax), LS_N), np.uint64)
        self._stat_rounds("list_stats", lambda t0, T, enabled: self.mc_batch_list(seed, t0, T, 1, ax, Ls, enabled, stats, constellation),
                          stats, LS_ERR, LS_RUN, max_runs, max_err, batch)
        run = np.maximum(stats[:, :, LS_RUN], 1).astype(np.float64)
        res = {"stats": stats}
        for name, col in (("bler", LS_ERR), ("miss_rate", LS_MISS), ("undetected_rate", LS_UNDET), ("ml_bound", LS_ML)):
            res[name] = stats[:, :, col] / run
        return res

    @staticmethod
    def _schedule(schedule):
        """A schedule of list sizes as the uint8 array the C-ABI takes (values out of uint8's range are refused here: the
        conversion would wrap them)."""
        v = [int(x) for x in np.atleast_1d(np.asarray(schedule)).tolist()]
        if any(not 0 <= x <= 255 for x in v):
            raise PolarError("list size out of range [1, 64] in schedule %r" % (v,))
        return np.array(v, np.uint8)

    def decode_scl_llr_adaptive(self, llr, schedule=(1, 4, 32), fmt=None, systematic=False):
        """Adaptive list decoding (polar_decode_scl_llr_adaptive_batch): every row is decoded with the list sizes of `schedule`
        (strictly increasing, at most 8, each 1 .. 64) in turn until the winner passes the CRC. Returns (out [B, K] uint8, pm [B]
        float64, stage [B] uint8, crc_ok [B] uint8): the word, its metric, the stage that delivered it and whether that stage
        accepted it (0 only at the last stage). out equals decode_scl_llr at the list size schedule[stage]. `llr` and `fmt` as
        decode_scl_llr_list; a single row [N] is a batch of one. The code needs a CRC.
        systematic=True: `out` is the message of the delivered word (systematic_message)."""
        code, a = _llr_rows(llr, fmt)
        a2 = a.reshape(-1, self.N)
        B, Ls = a2.shape[0], self._schedule(schedule)
        out = np.zeros((B, self.K), np.uint8)
        pm = np.zeros(B, np.float64)
        stage = np.zeros(B, np.uint8)
        crc_ok = np.zeros(B, np.uint8)
        self._chk(self._L.polar_decode_scl_llr_adaptive_batch(
            self._h, C.c_void_p(a2.ctypes.data), C.c_int(code), C.c_long(B), _p(Ls, _u8p), C.c_int(len(Ls)), _p(out, _u8p),
            C.c_void_p(pm.ctypes.data), C.c_void_p(stage.ctypes.data), C.c_void_p(crc_ok.ctypes.data)))
        if systematic:
            out = self.systematic_message(out)
        return out, pm, stage, crc_ok

    def decode_scl_llr_adaptive_dev(self, llr_ptr, fmt, B, schedule, out_ptr, pm_ptr=0, stage_ptr=0, crc_ok_ptr=0, stream=None):
        """Device-resident form (polar_decode_scl_llr_adaptive_batch_dev): LLRs [B, N] of format `fmt` -> out uint8 [B, K] and,
        where a pointer is given, pm float64 [B], stage uint8 [B], crc_ok uint8 [B]; asynchronous on `stream`, no host
        synchronisation between the stages."""
        Ls = self._schedule(schedule)
        self._chk(self._L.polar_decode_scl_llr_adaptive_batch_dev(
            self._h, C.c_void_p(llr_ptr), C.c_int(_llr_fmt_code(fmt)), C.c_long(B), _p(Ls, _u8p), C.c_int(len(Ls)),
            C.c_void_p(out_ptr), C.c_void_p(pm_ptr), C.c_void_p(stage_ptr), C.c_void_p(crc_ok_ptr), _stream_ptr(stream)))

    def mc_batch_adaptive(self, seed, t0, T, stride, axis, schedule, enabled, stats, constellation=0):
        """polar_mc_batch_adaptive: the trials {t0 + i*stride : i < T} of every enabled point ADD to stats, uint64
        [len(axis), 3 + len(schedule)] = AD_RUN, AD_ERR, AD_UNDET, then the trials delivered by each stage. constellation 0: BPSK,
        `axis` = Eb/N0 in dB; an ASK constellation: the BICM front end, `axis` = SNR in dB."""
        Ls = self._schedule(schedule)
        self._mc_batch_cells(self._L.polar_mc_batch_adaptive, seed, t0, T, stride, axis, Ls, enabled, stats, constellation,
                             AD_STAGE0 + len(Ls), False)

    def adaptive_stats(self, axis, schedule, max_runs=1000, max_err=100, seed=0, batch=0, constellation=0):
        """The adaptive decoder over a sweep: rounds of mc_batch_adaptive, sized and stopped like list_stats' (_stat_rounds). Returns a
        dict: `stats` uint64 [len(axis), 3 + len(schedule)] (AD_* columns), `bler` and `undetected_rate` = ERR and UNDET over RUN
        [len(axis)], `stage_share` [len(axis), len(schedule)] = the share of the trials each stage delivered, and `mean_effort`
        [len(axis)] = the mean over the trials of schedule[0] + ... + schedule[stage]: the list sizes a codeword went through
        (a fixed list of L costs L)."""
        ax = np.ascontiguousarray(axis, np.float64)
        Ls = self._schedule(schedule)
        stats = np.zeros((len(ax), AD_STAGE0 + len(Ls)), np.uint64)
        self._stat_rounds("adaptive_stats", lambda t0, T, enabled: self.mc_batch_adaptive(seed, t0, T, 1, ax, Ls, enabled, stats, constellation),
                          stats, AD_ERR, AD_RUN, max_runs, max_err, batch)
        run = np.maximum(stats[:, AD_RUN], 1).astype(np.float64)
        share = stats[:, AD_STAGE0:] / run[:, None]
        return {"stats": stats, "bler": stats[:, AD_ERR] / run, "undetected_rate": stats[:, AD_UNDET] / run, "stage_share": share,
                "mean_effort": share @ np.cumsum(Ls.astype(np.float64))}

    def decode_sc_flip(self, llr, max_flips=8, fmt=None, return_candidates=False, systematic=False):
        """SC-Flip (polar_decode_sc_flip_batch): one plain SC pass; while the word fails the CRC, whole re-decodes with one decision
        inverted — the `max_flips` (0 .. 64) unfrozen leaves of smallest |LLR| of the first pass, least reliable first. Returns (out
        [B, K] uint8, crc_ok [B] uint8, n_dec [B] uint8, flip [B] int32): the delivered word, whether it passed the CRC, the passes it
        took and the flipped position in decoding order (-1: none). return_candidates=True adds (cand [B, max_flips] int32, mag
        [B, max_flips] float64): pass 0's candidates and their magnitudes (-1 / inf past K + crc). `llr` and `fmt` as
        decode_scl_llr_list; a single row [N] is a batch of one. The code needs a CRC; n <= 12.
        systematic=True: `out` is the message of the delivered word (systematic_message)."""
        code, a = _llr_rows(llr, fmt)
        a2 = a.reshape(-1, self.N)
        B, T = a2.shape[0], int(max_flips)
        out = np.zeros((B, self.K), np.uint8)
        crc_ok = np.zeros(B, np.uint8)
        n_dec = np.zeros(B, np.uint8)
        flip = np.zeros(B, np.int32)
        cand = np.zeros((B, max(T, 0)), np.int32)
        mag = np.zeros((B, max(T, 0)), np.float64)
        self._chk(self._L.polar_decode_sc_flip_batch(
            self._h, C.c_void_p(a2.ctypes.data), C.c_int(code), C.c_long(B), C.c_int(T), _p(out, _u8p), C.c_void_p(crc_ok.ctypes.data),
            C.c_void_p(n_dec.ctypes.data), C.c_void_p(flip.ctypes.data), C.c_void_p(cand.ctypes.data if return_candidates else 0),
            C.c_void_p(mag.ctypes.data if return_candidates else 0)))
        if systematic:
            out = self.systematic_message(out)
        return (out, crc_ok, n_dec, flip, cand, mag) if return_candidates else (out, crc_ok, n_dec, flip)

    def decode_sc_flip_dev(self, llr_ptr, fmt, B, max_flips, out_ptr, crc_ok_ptr=0, n_dec_ptr=0, flip_ptr=0, cand_ptr=0, mag_ptr=0,
                           stream=None):
        """Device-resident form (polar_decode_sc_flip_batch_dev): LLRs [B, N] of format `fmt` -> out uint8 [B, K] and, where a pointer
        is given, crc_ok uint8 [B], n_dec uint8 [B], flip int32 [B], cand int32 [B, max_flips], mag float64 [B, max_flips];
        asynchronous on `stream`, one launch."""
        self._chk(self._L.polar_decode_sc_flip_batch_dev(
            self._h, C.c_void_p(llr_ptr), C.c_int(_llr_fmt_code(fmt)), C.c_long(B), C.c_int(max_flips), C.c_void_p(out_ptr),
            C.c_void_p(crc_ok_ptr), C.c_void_p(n_dec_ptr), C.c_void_p(flip_ptr), C.c_void_p(cand_ptr), C.c_void_p(mag_ptr),
            _stream_ptr(stream)))

    def mc_batch_flip(self, seed, t0, T, stride, axis, max_flips, enabled, stats, constellation=0):
        """polar_mc_batch_flip: the trials {t0 + i*stride : i < T} of every enabled point ADD to stats, uint64 [len(axis), 6] =
        FL_RUN, FL_ERR, FL_UNDET, FL_FIRST, FL_FLIPPED, FL_DECODES. constellation 0: BPSK, `axis` = Eb/N0 in dB; an ASK constellation:
        the BICM front end, `axis` = SNR in dB."""
        ax = np.ascontiguousarray(axis, np.float64)
        enabled = np.ascontiguousarray(enabled, np.uint8)
        if stats.dtype != np.uint64 or stats.size != len(ax) * FL_N or not stats.flags.c_contiguous:
            raise PolarError("stats must be a C-contiguous uint64 array [len(axis), %d]" % FL_N)
        if enabled.size != len(ax):
            raise PolarError("enabled must have len(axis) entries")
        self._chk(self._L.polar_mc_batch_flip(self._h, C.c_int(_constellation_id(constellation)), C.c_uint64(seed), C.c_uint64(t0),
                                              C.c_long(T), C.c_long(stride), _p(ax, _dp), C.c_int(len(ax)), C.c_int(max_flips),
                                              _p(enabled, _u8p), _p(stats, _u64p)))

    def flip_stats(self, axis, max_flips=8, max_runs=1000, max_err=100, seed=0, batch=0, constellation=0):
        """The SC-Flip decoder over a sweep: rounds of mc_batch_flip, sized and stopped like list_stats' (_stat_rounds). Returns a dict:
        `stats` uint64 [len(axis), 6] (FL_* columns), `bler`, `undetected_rate`, `first_share`, `flipped_share` = ERR, UNDET, FIRST,
        FLIPPED over RUN, and `mean_decodes` = DECODES over RUN: the SC passes a codeword took on average, all float64 [len(axis)]."""
        ax = np.ascontiguousarray(axis, np.float64)
        stats = np.zeros((len(ax), FL_N), np.uint64)
        self._stat_rounds("flip_stats", lambda t0, T, enabled: self.mc_batch_flip(seed, t0, T, 1, ax, max_flips, enabled, stats, constellation),
                          stats, FL_ERR, FL_RUN, max_runs, max_err, batch)
        run = np.maximum(stats[:, FL_RUN], 1).astype(np.float64)
        res = {"stats": stats}
        for name, col in (("bler", FL_ERR), ("undetected_rate", FL_UNDET), ("first_share", FL_FIRST), ("flipped_share", FL_FLIPPED),
                          ("mean_decodes", FL_DECODES)):
            res[name] = stats[:, col] / run
        return res

    def decode_scan(self, llr, iters=4, fmt=None, minsum=False, early_stop=False, systematic=False):
        """SCAN soft-output decoding (polar_decode_scan_batch): the SC schedule with LLRs passed in both directions, `iters` (1 .. 32)
        times. Returns (out [B, K] uint8, info_llr [B, K] float64, ext [B, N] float64, crc_ok [B] uint8, n_iter [B] uint8): the hard
        word, the LLRs of the info bits (out = info_llr < 0), the extrinsic LLRs of the coded bits, indexed like the row (+inf where
        the frozen set alone fixes a bit; a posteriori: llr + ext), whether the decided check bits are the CRC's (1 without a CRC),
        and the iterations that ran. minsum: f(a, b) = sgn sgn min instead of the f-node of decode_scl_llr; early_stop (needs a CRC):
        the first iteration whose decisions pass the CRC is the last. `llr` and `fmt` as decode_scl_llr_list; a single row [N] is a
        batch of one. Rows must be finite; n <= 11.
        systematic=True: `out` is the message of the hard word (systematic_message) and, in place of info_llr, msg_llr [B, K] =
        (llr + ext)[:, pos] comes back: the a-posteriori LLRs of the message bits (systematic_soft)."""
        code, a = _llr_rows(llr, fmt)
        a2 = a.reshape(-1, self.N)
        B = a2.shape[0]
        out = np.zeros((B, self.K), np.uint8)
        info_llr = np.zeros((B, self.K), np.float64)
        ext = np.zeros((B, self.N), np.float64)
        crc_ok = np.zeros(B, np.uint8)
        n_iter = np.zeros(B, np.uint8)
        self._chk(self._L.polar_decode_scan_batch(
            self._h, C.c_void_p(a2.ctypes.data), C.c_int(code), C.c_long(B), C.c_int(iters), C.c_int(_scan_flags(minsum, early_stop)),
            _p(out, _u8p), C.c_void_p(info_llr.ctypes.data), C.c_void_p(ext.ctypes.data), C.c_void_p(crc_ok.ctypes.data),
            C.c_void_p(n_iter.ctypes.data)))
        if systematic:
            out, info_llr = self.systematic_message(out), self.systematic_soft(a2, ext, code)
        return out, info_llr, ext, crc_ok, n_iter

    def decode_scan_dev(self, llr_ptr, fmt, B, iters, out_ptr, info_llr_ptr=0, ext_ptr=0, crc_ok_ptr=0, n_iter_ptr=0, minsum=False,
                        early_stop=False, stream=None):
        """Device-resident form (polar_decode_scan_batch_dev): LLRs [B, N] of format `fmt` -> out uint8 [B, K] and, where a pointer is
        given, info_llr float64 [B, K], ext float64 [B, N], crc_ok uint8 [B], n_iter uint8 [B]; asynchronous on `stream`, one launch."""
        self._chk(self._L.polar_decode_scan_batch_dev(
            self._h, C.c_void_p(llr_ptr), C.c_int(_llr_fmt_code(fmt)), C.c_long(B), C.c_int(iters), C.c_int(_scan_flags(minsum, early_stop)),
            C.c_void_p(out_ptr), C.c_void_p(info_llr_ptr), C.c_void_p(ext_ptr), C.c_void_p(crc_ok_ptr), C.c_void_p(n_iter_ptr),
            _stream_ptr(stream)))

    def mc_batch_scan(self, seed, t0, T, stride, axis, iters, enabled, stats, minsum=False, early_stop=False, constellation=0):
        """polar_mc_batch_scan: the trials {t0 + i*stride : i < T} of every enabled point ADD to stats, uint64 [len(axis), 4] = SN_RUN,
        SN_ERR, SN_UNDET, SN_ITERS. constellation 0: BPSK, `axis` = Eb/N0 in dB; an ASK constellation: the BICM front end, `axis` =
        SNR in dB."""
        ax = np.ascontiguousarray(axis, np.float64)
        enabled = np.ascontiguousarray(enabled, np.uint8)
        if stats.dtype != np.uint64 or stats.size != len(ax) * SN_N or not stats.flags.c_contiguous:
            raise PolarError("stats must be a C-contiguous uint64 array [len(axis), %d]" % SN_N)
        if enabled.size != len(ax):
            raise PolarError("enabled must have len(axis) entries")
        self._chk(self._L.polar_mc_batch_scan(self._h, C.c_int(_constellation_id(constellation)), C.c_uint64(seed), C.c_uint64(t0),
                                              C.c_long(T), C.c_long(stride), _p(ax, _dp), C.c_int(len(ax)), C.c_int(iters),
                                              C.c_int(_scan_flags(minsum, early_stop)), _p(enabled, _u8p), _p(stats, _u64p)))

    def scan_stats(self, axis, iters=4, max_runs=1000, max_err=100, seed=0, batch=0, constellation=0, minsum=False, early_stop=False):
        """The SCAN decoder over a sweep: rounds of mc_batch_scan, sized and stopped like list_stats' (_stat_rounds). Returns a dict:
        `stats` uint64 [len(axis), 4] (SN_* columns), `bler`, `undetected_rate` = ERR, UNDET over RUN, and `mean_iters` = ITERS over
        RUN: the iterations a codeword took on average, all float64 [len(axis)]."""
        ax = np.ascontiguousarray(axis, np.float64)
        stats = np.zeros((len(ax), SN_N), np.uint64)
        self._stat_rounds("scan_stats", lambda t0, T, enabled: self.mc_batch_scan(seed, t0, T, 1, ax, iters, enabled, stats, minsum,
                                                                                   early_stop, constellation),
                          stats, SN_ERR, SN_RUN, max_runs, max_err, batch)
        run = np.maximum(stats[:, SN_RUN], 1).astype(np.float64)
        res = {"stats": stats}
        for name, col in (("bler", SN_ERR), ("undetected_rate", SN_UNDET), ("mean_iters", SN_ITERS)):
            res[name] = stats[:, col] / run
        return res

    def decode_scl_llr_dev_f32(self, llr_ptr, B, list_size, out_ptr, pm_ptr=0, stream=None):
        """Device-resident float32 LLRs [B, N] -> uint8 [B, K]; asynchronous on `stream`."""
        self._chk(self._L.polar_decode_scl_llr_batch_dev_f32(self._h, C.c_void_p(llr_ptr), C.c_long(B), C.c_int(list_size),
                                                        C.c_void_p(out_ptr), C.c_void_p(pm_ptr), _stream_ptr(stream)))

    def decode_scl_llr_dev_fmt(self, llr_ptr, fmt, B, list_size, out_ptr, pm_ptr=0, stream=None):
        """Device-resident LLRs [B, N] of element format `fmt` ("f64", "f32", "f16", "bf16" or a POLAR_LLR_* code) -> uint8
        [B, K]; asynchronous on `stream`. A torch.float16 / torch.bfloat16 tensor's data_ptr() is what "f16" / "bf16" take."""
        self._chk(self._L.polar_decode_scl_llr_batch_dev_fmt(self._h, C.c_void_p(llr_ptr), C.c_int(_llr_fmt_code(fmt)), C.c_long(B),
                                                        C.c_int(list_size), C.c_void_p(out_ptr), C.c_void_p(pm_ptr),
                                                        _stream_ptr(stream)))

    def decode_scl_p1(self, p1, p0, list_size):
        """PolarCode::decode_scl_p1 (PolarCode.cpp:110-128)."""
        a = np.ascontiguousarray(p1, np.float64)
        b = np.ascontiguousarray(p0, np.float64)
        single = a.ndim == 1
        a2, b2 = a.reshape(-1, self.N), b.reshape(-1, self.N)
        out = np.zeros((a2.shape[0], self.K), np.uint8)
        self._chk(self._L.polar_decode_scl_p1_batch(self._h, _p(a2, _dp), _p(b2, _dp), C.c_long(a2.shape[0]),
                                               C.c_int(list_size), _p(out, _u8p)))
        return out[0] if single else out

    def decode_sc_p1(self, p1):
        """PolarM decode_sc_p1 (PolarCode.m:290-295)."""
        a = np.ascontiguousarray(p1, np.float64)
        single = a.ndim == 1
        a2 = a.reshape(-1, self.N)
        out = np.zeros((a2.shape[0], self.K), np.float64)
        self._chk(self._L.polar_decode_sc_p1_batch(self._h, _p(a2, _dp), C.c_long(a2.shape[0]), _p(out, _dp)))
        return out[0] if single else out

    # ---- multi-level coding receiver (PolarM/main_MC_CC_Comparison.m:55-62, 98-110) ---------
    def encode_mlc(self, info, constellation):
        """MLC encoder: info [B][K] (or [K]) -> coded bits [B][N] in modulation order (symbol i carries label bit k at
        i*nb + k; component k = message positions k*M .. (k+1)*M - 1, M = N / nb)."""
        a = np.ascontiguousarray(info, np.uint8)
        single = a.ndim == 1
        a2 = a.reshape(-1, self.K)
        out = np.zeros((a2.shape[0], self.N), np.uint8)
        self._chk(self._L.polar_encode_mlc(self._h, C.c_int(_constellation_id(constellation)), _p(a2, _u8p),
                                           C.c_long(a2.shape[0]), _p(out, _u8p)))
        return out[0] if single else out

    def decode_mlc(self, y, n0, constellation):
        """Multistage SC decoding of received symbols y [B][M] (or [M]) with noise variance n0 (= sigma^2): the K info
        decisions as doubles, decode_sc_p1's convention (0.5 / NaN where a leaf is undecided)."""
        cid = _constellation_id(constellation)
        a = np.ascontiguousarray(y, np.float64)
        single = a.ndim == 1
        nb = _NBITS.get(cid, 0)
        if nb and self.N % nb == 0:
            # (the library copies B * M doubles from the caller's rows: a row of any other width is refused here; an unknown
            # constellation or an N that nb does not divide is refused by the library before it reads anything)
            M = self.N // nb
            if a.ndim not in (1, 2) or a.shape[-1] != M:
                raise PolarError(f"decode_mlc: y must be [B][{M}] or [{M}] (M = N / n_bits = {self.N} / {nb}), got shape {a.shape}")
        a2 = a.reshape(1, -1) if single else a
        out = np.zeros((a2.shape[0], self.K), np.float64)
        self._chk(self._L.polar_decode_mlc(self._h, C.c_int(cid), _p(a2, _dp), C.c_double(n0), C.c_long(a2.shape[0]),
                                           _p(out, _dp)))
        return out[0] if single else out

    def decode_mlc_dev(self, constellation, y_ptr, n0, B, out_ptr, stream=None):
        self._chk(self._L.polar_decode_mlc_dev(self._h, C.c_int(_constellation_id(constellation)), C.c_void_p(y_ptr),
                                               C.c_double(n0), C.c_long(B), C.c_void_p(out_ptr), _stream_ptr(stream)))

    def synth_mlc_dev(self, constellation, seed, trial0, B, snr_db, y_ptr, info_ptr=0, stream=None):
        self._chk(self._L.polar_synth_mlc_dev(self._h, C.c_int(_constellation_id(constellation)), C.c_uint64(seed),
                                              C.c_uint64(trial0), C.c_long(B), C.c_double(snr_db), C.c_void_p(y_ptr),
                                              C.c_void_p(info_ptr), _stream_ptr(stream)))

    # ---- symbol-domain BICM receiver (Constellation.m:123-144 in front of decode_scl_llr) ---------
    def decode_bicm(self, y, n0, constellation, list_size, out=None):
        """decode_scl_llr from received symbols y [B][M] (or [M]), M = N // n_bits, with noise variance n0: bit for bit
        ``decode_scl_llr(Constellation(c).compute_llr_bicm(y, n0, N)[1], list_size)`` from 1 / n_bits of the input bytes —
        1 / (2 n_bits) for float32 symbols, which are widened exactly on the device. ``out`` as decode_scl_llr's."""
        cid = constellation.id if isinstance(constellation, Constellation) else _constellation_id(constellation)
        f32 = isinstance(y, np.ndarray) and y.dtype == np.float32
        a = np.ascontiguousarray(y) if f32 else np.ascontiguousarray(y, np.float64)
        single = a.ndim == 1
        nb = _NBITS.get(cid, 0)
        if nb:
            # (the library copies B * M elements from the caller's rows: a row of any other width is refused here; an unknown
            # constellation is refused by the library before it reads anything)
            M = self.N // nb
            if a.ndim not in (1, 2) or a.shape[-1] != M:
                raise PolarError(f"decode_bicm: y must be [B][{M}] or [{M}] (M = N // n_bits = {self.N} // {nb}), got shape {a.shape}")
        a2 = a.reshape(1, -1) if single else a
        B = a2.shape[0]
        if out is None:
            out = np.zeros((B, self.K), np.uint8)
        elif out.dtype != np.uint8 or out.shape != (B, self.K) or not out.flags.c_contiguous:
            raise PolarError("out must be a C-contiguous uint8 array of shape [B, K]")
        f = self._L.polar_decode_bicm_batch_f32 if f32 else self._L.polar_decode_bicm_batch
        self._chk(f(self._h, C.c_int(cid), _p(a2, C.POINTER(C.c_float) if f32 else _dp), C.c_double(n0), C.c_long(B),
                    C.c_int(list_size), _p(out, _u8p)))
        return out[0] if single else out

    def decode_bicm_dev(self, constellation, y_ptr, n0, B, list_size, out_ptr, pm_ptr=0, stream=None, f32=False):
        """Device-resident symbols [B][N // n_bits] (float64, or float32 with f32=True) -> uint8 [B][K]; asynchronous on
        `stream`, path metrics as decode_scl_llr_dev."""
        cid = constellation.id if isinstance(constellation, Constellation) else _constellation_id(constellation)
        f = self._L.polar_decode_bicm_batch_dev_f32 if f32 else self._L.polar_decode_bicm_batch_dev
        self._chk(f(self._h, C.c_int(cid), C.c_void_p(y_ptr), C.c_double(n0), C.c_long(B), C.c_int(list_size),
                    C.c_void_p(out_ptr), C.c_void_p(pm_ptr), _stream_ptr(stream)))

    def synth_bicm_sym_dev(self, constellation, seed, trial0, B, snr_db, y_ptr, info_ptr=0, stream=None):
        """The received symbols [B][N // n_bits] of the trials synth_bicm_llr_dev gives the LLRs of."""
        self._chk(self._L.polar_synth_bicm_sym_dev(self._h, C.c_int(_constellation_id(constellation)), C.c_uint64(seed),
                                                   C.c_uint64(trial0), C.c_long(B), C.c_double(snr_db), C.c_void_p(y_ptr),
                                                   C.c_void_p(info_ptr), _stream_ptr(stream)))

    # names used by BASELINE.json's north_star
    decode_SCL_LLR = decode_scl_llr
    decode_SCL_P1 = decode_scl_p1
    decode_SC_P1 = decode_sc_p1

    # ---- device-resident entry points (torch tensors are only memory + stream plumbing) ---
    def decode_scl_llr_dev(self, llr_ptr, B, list_size, out_ptr, pm_ptr=0, stream=None, ev_start=0, ev_stop=0):
        """ev_start / ev_stop: raw hipEvent_t handles (e.g. torch.cuda.Event(...).cuda_event) recorded
        immediately around the dominant kernel's launch."""
        self._chk(self._L.polar_decode_scl_llr_batch_dev_ev(self._h, C.c_void_p(llr_ptr), C.c_long(B), C.c_int(list_size),
                                                       C.c_void_p(out_ptr), C.c_void_p(pm_ptr), _stream_ptr(stream),
                                                       C.c_void_p(ev_start), C.c_void_p(ev_stop)))

    def synth_llr_dev(self, seed, trial0, B, s, llr_ptr, info_ptr=0, stream=None):
        self._chk(self._L.polar_synth_llr_dev(self._h, C.c_uint64(seed), C.c_uint64(trial0), C.c_long(B), C.c_double(s),
                                         C.c_void_p(llr_ptr), C.c_void_p(info_ptr), _stream_ptr(stream)))

    def count_errors_dev(self, a_ptr, b_ptr, B, counter_ptr, stream=None):
        self._chk(self._L.polar_count_errors_dev(self._h, C.c_void_p(a_ptr), C.c_void_p(b_ptr), C.c_long(B),
                                            C.c_void_p(counter_ptr), _stream_ptr(stream)))

    def encode_dev(self, info_ptr, B, coded_ptr, stream=None):
        self._chk(self._L.polar_encode_batch_dev(self._h, C.c_void_p(info_ptr), C.c_long(B), C.c_void_p(coded_ptr),
                                            _stream_ptr(stream)))

    # ---- Monte-Carlo (PolarCode.cpp:658-785) ---------------------------------------------
    def mc_batch(self, seed, t0, T, stride, ebno_vec, list_size_vec, enabled, err, run):
        ebno = np.ascontiguousarray(ebno_vec, np.float64)
        Ls = np.ascontiguousarray(list_size_vec, np.uint8)
        enabled = np.ascontiguousarray(enabled, np.uint8)
        assert err.dtype == np.uint64 and run.dtype == np.uint64
        self._chk(self._L.polar_mc_batch(self._h, C.c_uint64(seed), C.c_uint64(t0), C.c_long(T), C.c_long(stride),
                                    _p(ebno, _dp), C.c_int(len(ebno)), _p(Ls, _u8p), C.c_int(len(Ls)),
                                    _p(enabled, _u8p), _p(err, _u64p), _p(run, _u64p)))

    def synth_bicm_llr_dev(self, constellation, seed, trial0, B, snr_db, llr_ptr, info_ptr=0, stream=None):
        self._chk(self._L.polar_synth_bicm_llr_dev(self._h, C.c_int(_constellation_id(constellation)), C.c_uint64(seed), C.c_uint64(trial0),
                                              C.c_long(B), C.c_double(snr_db), C.c_void_p(llr_ptr),
                                              C.c_void_p(info_ptr), _stream_ptr(stream)))

    def mc_batch_bicm(self, constellation, seed, t0, T, stride, snr_db_vec, list_size_vec, enabled, err, run):
        snr = np.ascontiguousarray(snr_db_vec, np.float64)
        Ls = np.ascontiguousarray(list_size_vec, np.uint8)
        enabled = np.ascontiguousarray(enabled, np.uint8)
        assert err.dtype == np.uint64 and run.dtype == np.uint64
        self._chk(self._L.polar_mc_batch_bicm(self._h, C.c_int(_constellation_id(constellation)), C.c_uint64(seed), C.c_uint64(t0), C.c_long(T),
                                         C.c_long(stride), _p(snr, _dp), C.c_int(len(snr)), _p(Ls, _u8p),
                                         C.c_int(len(Ls)), _p(enabled, _u8p), _p(err, _u64p), _p(run, _u64p)))

    def mc_batch_ber(self, seed, t0, T, stride, ebno_vec, list_size_vec, enabled, err, bit_err, run):
        ebno = np.ascontiguousarray(ebno_vec, np.float64)
        Ls = np.ascontiguousarray(list_size_vec, np.uint8)
        enabled = np.ascontiguousarray(enabled, np.uint8)
        assert err.dtype == np.uint64 and run.dtype == np.uint64 and bit_err.dtype == np.uint64
        self._chk(self._L.polar_mc_batch_ber(self._h, C.c_uint64(seed), C.c_uint64(t0), C.c_long(T), C.c_long(stride),
                                        _p(ebno, _dp), C.c_int(len(ebno)), _p(Ls, _u8p), C.c_int(len(Ls)),
                                        _p(enabled, _u8p), _p(err, _u64p), _p(bit_err, _u64p), _p(run, _u64p)))

    def get_bler_quick(self, ebno_vec, list_size_vec, max_runs=1000, max_err=100, seed=1, batch=None,
                       return_ber=False, devices=None, constellation=None, return_counters=False, receiver="bicm"):
        """PolarCode::get_bler_quick: returns bler[len(list_size_vec)][len(ebno_vec)] (PolarCode.cpp:658-785);
        with return_ber=True also PolarM's second output ber (PolarCode.m:781,848), same layout.
        batch=None: the library picks the rounds (see polar_amd.h). devices=[...]: shard the trials over these GPUs
        of the node from this one process (polar_get_bler_quick_multi_ex, RCCL all-reduce of the counters, one per round).
        constellation="ask16-gray" (...): the ASK Gray + BICM front end with `ebno_vec` read as the SNR axis in dB
        (PolarM/main_MC_CC_Comparison.m:44-119); receiver="mlc" with it: the multi-level coding receiver (list size 1).
        return_counters=True: additionally a dict with the raw counters err / run (uint64, same layout) and the number of
        rounds."""
        ebno = np.ascontiguousarray(ebno_vec, np.float64)
        Ls = np.ascontiguousarray(list_size_vec, np.uint8)
        shape = (len(Ls), len(ebno))
        out = np.zeros(shape, np.float64)
        ber = np.zeros(shape, np.float64)
        err = np.zeros(shape, np.uint64)
        run = np.zeros(shape, np.uint64)
        if batch is None:
            batch = 0
        cid = _sweep_id(constellation, receiver)
        if devices is not None:
            devs = np.ascontiguousarray(devices, np.int32)
            dptr, nd = devs.ctypes.data_as(C.POINTER(C.c_int)), len(devs)
        else:
            dptr, nd = None, 1
        used, rounds = C.c_int(0), C.c_long(0)
        self._chk(self._L.polar_get_bler_quick_multi_ex(self._h, C.c_int(cid), dptr, C.c_int(nd),
                                                   _p(ebno, _dp), C.c_int(len(ebno)), _p(Ls, _u8p), C.c_int(len(Ls)),
                                                   C.c_long(max_runs), C.c_long(max_err), C.c_uint64(seed), C.c_long(batch),
                                                   _p(out, _dp), _p(ber, _dp), _p(err, _u64p), _p(run, _u64p),
                                                   C.byref(rounds), C.byref(used)))
        self.last_used_rccl = bool(used.value)
        res = (out, ber) if return_ber else (out,)
        if return_counters:
            res = res + ({"err": err, "run": run, "rounds": int(rounds.value)},)
        return res[0] if len(res) == 1 else res

    def get_bler_quick_rank(self, ebno_vec, list_size_vec, rank, world, reduce, max_runs=1000, max_err=100, seed=1, batch=None,
                            constellation=None, receiver="bicm"):
        """polar_get_bler_quick_rank: this process is `rank` of `world` sharing the sweep; `reduce(a)` must SUM the uint64 numpy
        array `a` in place over the ranks (called collectively after every step). Returns (bler, ber, counters) like
        get_bler_quick(..., return_ber=True, return_counters=True)."""
        ebno = np.ascontiguousarray(ebno_vec, np.float64)
        Ls = np.ascontiguousarray(list_size_vec, np.uint8)
        shape = (len(Ls), len(ebno))
        out, ber = np.zeros(shape, np.float64), np.zeros(shape, np.float64)
        err, run = np.zeros(shape, np.uint64), np.zeros(shape, np.uint64)
        rounds = C.c_long(0)
        failure = []

        @C.CFUNCTYPE(C.c_int, C.c_void_p, _u64p, C.c_int)
        def cb(_user, ptr, n):
            try:
                a = np.ctypeslib.as_array(ptr, shape=(n,))
                reduce(a)
                return 0
            except Exception as ex:          # (no exception may cross the C frames)
                failure.append(ex)
                return 1
        cid = _sweep_id(constellation, receiver)
        rc = self._L.polar_get_bler_quick_rank(self._h, C.c_int(cid), C.c_int(rank), C.c_int(world), cb, None,
                                             _p(ebno, _dp), C.c_int(len(ebno)), _p(Ls, _u8p), C.c_int(len(Ls)),
                                             C.c_long(max_runs), C.c_long(max_err), C.c_uint64(seed), C.c_long(batch or 0),
                                             _p(out, _dp), _p(ber, _dp), _p(err, _u64p), _p(run, _u64p), C.byref(rounds))
        if failure:
            raise failure[0]
        _check(rc)
        return out, ber, {"err": err, "run": run, "rounds": int(rounds.value), "steps": self.debug_get("round_us_count")}


def _rm_scheme(scheme):
    if isinstance(scheme, str):
        if scheme not in RM_SCHEMES:
            raise PolarError(f"unknown rate-matching scheme {scheme!r} (supported: {sorted(RM_SCHEMES)})")
        return RM_SCHEMES[scheme]
    return int(scheme)


def rate_match_pattern(n, E, scheme, Kp=None):
    """(sel uint16 [E], known uint8 [N]) of a built-in scheme (polar_rm_pattern; host only): "puncture", "shorten", "repeat" or
    "nr" (Kp = K + crc decides between NR's puncturing and shortening)."""
    if E < 1:
        raise PolarError("rate_match_pattern: E must be positive")
    sel, known = np.zeros(int(E), np.uint16), np.zeros(1 << n if 0 < n < 31 else 1, np.uint8)
    _check(lib().polar_rm_pattern(C.c_int(n), C.c_int(E), C.c_int(_rm_scheme(scheme)), C.c_int(0 if Kp is None else Kp),
                                  _p(sel, _u16p), _p(known, _u8p)))
    return sel, known


def rate_match_forced(n, sel, known=None):
    """The leaves a design for this pattern must freeze, as a mask uint8 [N] by leaf index (polar_rm_forced; host only)."""
    sel = np.ascontiguousarray(sel, np.uint16).reshape(-1)
    kn = None if known is None else np.ascontiguousarray(known, np.uint8)
    forced = np.zeros(1 << n if 0 < n < 31 else 1, np.uint8)
    if kn is not None and kn.shape != forced.shape:
        raise PolarError("rate_match_forced: known must have N entries")
    _check(lib().polar_rm_forced(C.c_int(n), _p(sel, _u16p), C.c_int(sel.size), _p(kn, _u8p) if kn is not None else None,
                                 _p(forced, _u8p)))
    return forced


def ga_construction_init(num_layers, init, forced=None, phi_dx=1e-5):
    """polar_ga_construction_init: the Gaussian-approximation design started from init [n_points, N] (coded order) ->
    (channels [n_points, N], order uint16 [n_points, N], bler_prefix [n_points, N]); the leaves with forced[leaf] != 0 end every
    order row, in ascending index."""
    N = 1 << num_layers
    a = np.ascontiguousarray(init, np.float64)
    if a.ndim != 2 or a.shape[1] != N:
        raise PolarError("ga_construction_init: init must be [n_points, N]")
    f = None if forced is None else np.ascontiguousarray(forced, np.uint8)
    if f is not None and f.shape != (N,):
        raise PolarError("ga_construction_init: forced must have N entries")
    P = a.shape[0]
    ch, order, pre = np.zeros((P, N)), np.zeros((P, N), np.uint16), np.zeros((P, N))
    _check(lib().polar_ga_construction_init(C.c_int(num_layers), _p(a, _dp), _p(f, _u8p) if f is not None else None, C.c_int(P),
                                            C.c_double(phi_dx), _p(ch, _dp), _p(order, _u16p), _p(pre, _dp)))
    return ch, order, pre


def _sweep_id(constellation, receiver):
    flag = _rx_flag(receiver)
    if constellation is None:
        if flag:
            raise PolarError("the MLC receiver needs a constellation")
        return 0
    return _constellation_id(constellation) | flag


# ---- Monte-Carlo code construction (PolarM/PolarCode.m:95-196) ---------------------------------
def _num2str(x):
    """MATLAB num2str for the values the reference puts in file names (integers and short decimals)."""
    return str(int(x)) if float(x) == int(x) else ("%.4f" % float(x)).rstrip("0").rstrip(".")


def construction_unique_string(block_length, num_info_bits, design_snr_db, constellation_name="bpsk",
                               receiver_algo="bicm", num_runs=20000):
    """get_unique_string (PolarCode.m:258-261) for cc_method 'monte-carlo' (:107-109)."""
    return (f"{_num2str(block_length)}_{_num2str(num_info_bits)}_cc_method_monte-carlo_cc_param_"
            f"{_num2str(design_snr_db)}_{constellation_name}_{receiver_algo}_{_num2str(num_runs)}")


def write_construction_file(path, counts):
    """One count per line, '%d \n' (PolarCode.m:120-124)."""
    with open(path, "w") as f:
        for c in np.asarray(counts).reshape(-1):
            f.write("%d \n" % int(c))


def mc_construction(num_layers, design_snr_db, num_runs, constellation="bpsk", seed=1, trial0=0, batch=0, out=None,
                    receiver="bicm"):
    """Per-position error counts of the genie-aided SC decoder over ``num_runs`` Monte-Carlo runs
    (PolarCode.m:143-196 `monte_carlo`), computed on the GPU. Returns uint64[N];
    with ``out`` the counts are ADDED to it (shards of one trial range, see montecarlo.py).
    receiver="mlc": the genie-aided multistage decoder of the MLC receiver, counts layer-major (:155-161, 180-190)."""
    N = 1 << num_layers
    if out is None:
        out = np.zeros(N, np.uint64)
    if out.dtype != np.uint64 or out.shape != (N,) or not out.flags.c_contiguous:
        raise PolarError("out must be a contiguous uint64[N] array")
    _check(lib().polar_mc_construction(C.c_int(num_layers), C.c_int(_constellation_id(constellation) | _rx_flag(receiver)),
                                       C.c_double(design_snr_db), C.c_uint64(seed), C.c_uint64(trial0),
                                       C.c_long(num_runs), C.c_long(batch), _p(out, _u64p)))
    return out


# ---- Gaussian-approximation code construction (PolarM/PolarCode.m:198-255, main_GA_CC_Comparison.m) ---------------------
GA_CONSTELLATIONS = ("bpsk", "ask4-gray", "ask4-sp", "ask16-gray", "ask16-sp")   # 8-ASK: refused (include/polar_amd.h)
GA_BINS = 801                  # polarized capacity: u-LLR bins of width 0.25 over [-100, 100]


def _ga_id(constellation):
    cid = _constellation_id(constellation)
    if cid not in (BPSK, ASK4_GRAY, ASK4_SP, ASK16_GRAY, ASK16_SP):
        raise PolarError(f"constellation {constellation!r} is not supported by the GA construction (supported: {GA_CONSTELLATIONS})")
    return cid


def _snr_array(snr_db):
    return np.ascontiguousarray(np.atleast_1d(np.asarray(snr_db, np.float64)).reshape(-1))


def _capacity(fn, constellation, snr_db):
    cid = _ga_id(constellation)
    snr = _snr_array(snr_db)
    out = np.zeros((snr.size, _NBITS[cid]))
    _check(getattr(lib(), fn)(C.c_int(cid), _p(snr, _dp), C.c_int(snr.size), _p(out, _dp)))
    return out


def bicm_capacity(constellation, snr_db):
    """Constellation.get_bicm_capacity (Constellation.m:250-286) on the GPU: [len(snr_db)][n_bits]."""
    return _capacity("polar_bicm_capacity", constellation, snr_db)


def mlc_capacity(constellation, snr_db):
    """Constellation.get_mlc_capacity (Constellation.m:190-248) on the GPU: [len(snr_db)][n_bits], layer by layer."""
    return _capacity("polar_mlc_capacity", constellation, snr_db)


def bpsk_capacity(snr_db=None):
    """CapacityHelper/get_bpsk_cap.m on the GPU: [len(snr_db)]; None = the table of get_bpsk_llr_for_capacity.m
    (-20 : 0.01 : 20 dB as -20 + k * 0.01, 4001 points)."""
    snr = _snr_array(-20.0 + np.arange(4001) * 0.01 if snr_db is None else snr_db)
    out = np.zeros(snr.size)
    _check(lib().polar_bpsk_capacity(_p(snr, _dp), C.c_int(snr.size), _p(out, _dp)))
    return out


def ga_phi_tables(phi_dx=1e-5):
    """initialize_phi.m on the GPU: (forward table [10002], inverse table [100001])."""
    fwd, inv = np.zeros(10002), np.zeros(100001)
    _check(lib().polar_ga_phi_tables(C.c_double(phi_dx), _p(fwd, _dp), _p(inv, _dp)))
    return fwd, inv


def polarized_counts(constellation, snr_db, num_sym, seed=1, trial0=0, out=None):
    """u-LLR histograms of Constellation.get_polarized_capacity (Constellation.m:288-370) for symbols trial0 ..
    trial0+num_sym-1: uint64 [len(snr_db)][n_bits][801][2] (bin, sent bit). With ``out`` they are ADDED to it, so disjoint
    seeds or symbol ranges combine."""
    cid = _ga_id(constellation)
    snr = _snr_array(snr_db)
    shape = (snr.size, _NBITS[cid], GA_BINS, 2)
    if out is None:
        out = np.zeros(shape, np.uint64)
    if out.dtype != np.uint64 or out.shape != shape or not out.flags.c_contiguous:
        raise PolarError(f"out must be a contiguous uint64{list(shape)} array")
    _check(lib().polar_polarized_counts(C.c_int(cid), _p(snr, _dp), C.c_int(snr.size), C.c_long(num_sym), C.c_uint64(seed),
                                        C.c_uint64(trial0), _p(out, _u64p)))
    return out


def polarized_capacity_from_counts(constellation, counts):
    cid = _ga_id(constellation)
    counts = np.ascontiguousarray(counts, np.uint64)
    n = counts.shape[0]
    if counts.shape != (n, _NBITS[cid], GA_BINS, 2):
        raise PolarError("counts must be [n][n_bits][801][2]")
    out = np.zeros((n, _NBITS[cid]))
    _check(lib().polar_polarized_capacity_from_counts(C.c_int(cid), C.c_int(n), _p(counts, _u64p), _p(out, _dp)))
    return out


def polarized_capacity(constellation, snr_db, num_sym=250000, seed=1, data_dir=None):
    """Constellation.get_polarized_capacity on the GPU: [len(snr_db)][n_bits]. With ``data_dir`` each SNR is read from /
    written to ``<constellation>_snr_<num2str(snr)>.mat`` (variable cap_vec) as the reference does (:290-296, 367), which
    needs scipy; without scipy data_dir is refused."""
    snr = _snr_array(snr_db)
    name = constellation if isinstance(constellation, str) else \
        {v: k for k, v in CONSTELLATION_NAMES.items()}[_constellation_id(constellation)]
    if data_dir is None:
        return polarized_capacity_from_counts(constellation, polarized_counts(constellation, snr, num_sym, seed))
    try:
        import scipy.io
    except ImportError as e:
        raise PolarError("polarized_capacity(data_dir=...) reads and writes .mat files and needs scipy") from e
    out = np.zeros((snr.size, _NBITS[_ga_id(constellation)]))
    todo = []
    for i, s in enumerate(snr):
        path = os.path.join(data_dir, f"{name}_snr_{_num2str(s)}.mat")
        if os.path.exists(path):
            out[i] = scipy.io.loadmat(path)["cap_vec"].reshape(-1)[: out.shape[1]]
        else:
            todo.append(i)
    if todo:
        cap = polarized_capacity_from_counts(constellation, polarized_counts(constellation, snr[todo], num_sym, seed))
        for j, i in enumerate(todo):
            out[i] = cap[j]
            scipy.io.savemat(os.path.join(data_dir, f"{name}_snr_{_num2str(snr[i])}.mat"), {"cap_vec": cap[j].reshape(-1, 1)})
    return out


def ga_mean_llr(capacity):
    """get_bpsk_llr_for_capacity.m against the device's BPSK capacity table."""
    cap = np.ascontiguousarray(capacity, np.float64)
    out = np.zeros(cap.shape)
    _check(lib().polar_ga_mean_llr(_p(cap, _dp), C.c_int(cap.size), _p(out, _dp)))
    return out


def ga_construction(num_layers, snr_db, constellation="bpsk", receiver="bicm", phi_dx=1e-5, seed=1, capacity=None):
    """Gaussian-approximation construction of every design SNR in one launch (PolarCode.m:198-255): returns
    (channels [P][N], order [P][N] stable descending = most reliable first, bler_prefix [P][N]); bler_prefix[p][K-1] is the
    BLER estimate of the code with K unfrozen positions. ``capacity`` [P][n_bits] replaces the computed capacities."""
    cid = _ga_id(constellation)
    flag = _rx_flag(receiver)
    snr = _snr_array(snr_db)
    P, N = snr.size, 1 << num_layers
    cap = None
    if capacity is not None:
        cap = np.ascontiguousarray(capacity, np.float64)
        if cap.shape != (P, _NBITS[cid]):
            raise PolarError(f"capacity must be [{P}][{_NBITS[cid]}]")
    ch, order, pre = np.zeros((P, N)), np.zeros((P, N), np.uint16), np.zeros((P, N))
    _check(lib().polar_ga_construction(C.c_int(num_layers), C.c_int(cid | flag), _p(snr, _dp), C.c_int(P),
                                       C.c_double(phi_dx), C.c_uint64(seed), _p(cap, _dp) if cap is not None else None,
                                       _p(ch, _dp), _p(order, _u16p), _p(pre, _dp)))
    return ch, order, pre


def ga_rate_table(rates=(1 / 32, 1 / 16, 1 / 8, 1 / 4, 2 / 4, 3 / 4, 7 / 8),
                  constellations=("ask4-gray", "ask4-sp", "ask16-gray", "ask16-sp"), receivers=("bicm", "mlc", "bicm", "mlc"),
                  snr_db_vec=None, target_bler=1e-5, block_length=1024, phi_dx=1e-5, seed=1, capacities=None):
    """PolarM's main_GA_CC_Comparison.m on the GPU: one GA construction per (constellation, SNR), then per rate the
    reference's walk over the SNR grid (from the previous rate's stopping index minus one, until the estimate of
    K = ceil(rate * N) falls below the target) and its log interpolation. Returns a dict with ``snr_needed`` and
    ``ebno_needed`` [rate][constellation] and ``flags``. Deviation: where the reference waits for a key press ('Possibly
    too high starting SNR', flag 1, then interpolating with a stale estimate) or runs off the grid (flag 2), the entry is
    NaN. ``capacities`` (a list of [len(snr_db_vec)][n_bits] arrays or None per constellation) replaces computed ones."""
    if snr_db_vec is None:
        snr_db_vec = -10.0 + np.arange(161) * 0.25
    snr = _snr_array(snr_db_vec)
    n = int(round(np.log2(block_length)))
    Ks = [int(np.ceil(r * block_length)) for r in rates]
    shape = (len(rates), len(constellations))
    snr_needed, ebno, flags = np.full(shape, np.nan), np.full(shape, np.nan), np.zeros(shape, np.int64)
    for ci, (c, rx) in enumerate(zip(constellations, receivers)):
        cap = None if capacities is None else capacities[ci]
        _, _, pre = ga_construction(n, snr, c, rx, phi_dx, seed, cap)
        bler = pre[:, [k - 1 for k in Ks]]
        snr_needed[:, ci], ebno[:, ci], flags[:, ci] = _rate_walk(bler, rates, snr, target_bler, _NBITS[_ga_id(c)])
    return {"snr_needed": snr_needed, "ebno_needed": ebno, "flags": flags, "snr_db_vec": snr, "rates": np.asarray(rates)}


def _rate_walk(bler, rates, snr_vec, target, nbits):
    """main_GA_CC_Comparison.m:34-66 over bler[snr][rate] (see ga_rate_table)."""
    import math
    nr = len(rates)
    snr_needed, ebno, flags = np.full(nr, np.nan), np.full(nr, np.nan), np.zeros(nr, np.int64)
    start = 0
    for r in range(nr):
        idx, prev = None, None
        for si in range(start, len(snr_vec)):
            if bler[si, r] < target:
                idx = si
                break
            prev = bler[si, r]
        if idx is None:
            flags[r] = 2
            start = max(len(snr_vec) - 2, 0)
            continue
        if idx == start:
            flags[r] = 1
        else:
            b = bler[idx, r]
            snr_needed[r] = (snr_vec[idx] * math.log(prev / target) + snr_vec[idx - 1] * math.log(target / b)) / math.log(prev / b)
            ebno[r] = snr_needed[r] - 10 * math.log10(rates[r]) - 10 * math.log10(nbits)
        start = max(idx - 1, 0)
    return snr_needed, ebno, flags
