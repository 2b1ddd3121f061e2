// polar_flip.cpp — SC-Flip (include/polar_amd.h polar_decode_sc_flip_batch*): one plain SC pass; while the word fails the
// CRC, whole re-decodes with one decision inverted — the unfrozen leaves of smallest |LLR| of the first pass, least reliable first.
// One kernel (polar_kernels_flip.hip sc_flip_kernel), one launch for the whole batch: the retry loop runs in the kernel, the host
// chains nothing. The handle's mode, tuning and latency threshold are not looked at.
#include "polar_host.h"

namespace {

// what the decode and the sweep refuse alike, after their pointers
int flip_check_code(const polar_code *h, int max_flips) {
    if (max_flips < 0 || max_flips > POLAR_FLIP_MAX) return fail(POLAR_E_ARG, "max_flips %d out of range [0, %d]", max_flips, POLAR_FLIP_MAX);
    return h->crc ? POLAR_OK : fail(POLAR_E_ARG, "SC-Flip needs a CRC: this code has none to accept a word on");
}
int flip_check_size(const polar_code *h) {
    return h->n > polar_flip_max_log() ? fail(POLAR_E_UNSUPPORTED, "SC-Flip keeps a codeword in LDS: n = %d is above %d", h->n, polar_flip_max_log()) : POLAR_OK;
}
int flip_check(const polar_code *h, const void *llr, int fmt, long B, int max_flips, const uint8_t *out) {
    if (!h || !llr || !out) return fail(POLAR_E_ARG, "NULL argument");
    if (int rc = flip_check_code(h, max_flips)) return rc;
    if (int rc = llr_fmt_check(fmt, llr)) return rc;
    if (B < 0) return fail(POLAR_E_ARG, "negative batch");
    return flip_check_size(h);
}

// The walk of sc_flip_kernel over the code tree, depth first; node v of layer lam covers the leaves [v << (n - lam), (v + 1) << (n - lam)).
// An all-frozen subtree has no ops; a node of four leaves is ONE op.
void flip_schedule(polar_code *h) {
    const int n = h->n;
    const LeafCount unf(h);
    auto brev = [](int v, int bits) { int r = 0; for (int i = 0; i < bits; ++i) r |= ((v >> i) & 1) << (bits - 1 - i); return r; };
    auto emit = [&](int type, int lam, int arg) { h->flip_ops.push_back((uint32_t)type | ((uint32_t)lam << 3) | ((uint32_t)arg << 8)); };
    std::function<void(int, int)> go = [&](int lam, int v) {
        auto live = [&](int l, int w) { return unf.under(l, w) > 0; };
        if (lam == n - 2 || lam == n - 1) {                                       // (n - 1: only the root of n = 1)
            const int size = 1 << (n - lam);
            int arg = size * v;
            for (int i = 0; i < size; ++i) arg |= (h->frozen[size * v + i] ? 1 : 0) << (16 + i);
            emit(size == 4 ? POLAR_FLIP_OP_QUAD : POLAR_FLIP_OP_PAIR, lam, arg);
            return;
        }
        if (live(lam + 1, 2 * v)) { emit(POLAR_FLIP_OP_F, lam + 1, 0); go(lam + 1, 2 * v); }
        if (live(lam + 1, 2 * v + 1)) { emit(POLAR_FLIP_OP_G, lam + 1, brev(2 * v, lam + 1)); go(lam + 1, 2 * v + 1); }
        if (lam > 0) emit(POLAR_FLIP_OP_COMBINE, lam + 1, brev(v, lam));
    };
    h->flip_ops.clear();
    go(0, 0);                                                                      // (K >= 1: the root is never all frozen)
}

int flip_prepare(polar_code *h) {
    return ops_prepare(h, polar_flip_lds_bytes(h->N), "the SC-Flip kernel's LDS does not fit this device", h->flip_ops, h->d_flip_ops, flip_schedule);
}

// (arguments checked, B > 0, the handle's device current, flip_prepare done)
int flip_launch(polar_code *h, const void *d_llr, int fmt, long B, int max_flips, uint8_t *d_out, uint8_t *d_crc_ok, uint8_t *d_n_dec,
                int32_t *d_flip, int32_t *d_cand, double *d_mag, hipStream_t st) {
    PolarFlipParams p;
    p.n = h->n; p.N = h->N; p.K = h->K; p.crc = h->crc; p.T = max_flips; p.B = B;
    p.llr = d_llr; p.llr_fmt = fmt; p.ops = h->d_flip_ops.p; p.n_ops = (int)h->flip_ops.size();
    p.order = h->d_order.p; p.crcm = h->d_crcm.p; p.tabs = h->d_tabs.p;
    p.out = d_out; p.crc_ok = d_crc_ok; p.n_dec = d_n_dec; p.flip = d_flip;
    p.cand = max_flips ? d_cand : nullptr; p.mag = max_flips ? d_mag : nullptr;
    HIP_TRY(polar_launch_sc_flip(p, (int)std::min<long>(B, polar_flip_grid_cap()), st));
    return POLAR_OK;
}

// One chunk of the host form's and the sweep's outputs: the magnitudes in d_list_out, flip and cand in d_flip_i32, the words in
// d_out, crc_ok and n_dec in d_bytes_b
struct FlipChunk {
    double *mag; int32_t *flip, *cand; uint8_t *out, *crc_ok, *n_dec;
    static int make(polar_code *h, long B, int T, FlipChunk &c) {
        int rc;
        if ((rc = h->d_list_out.ensure((size_t)B * std::max(T, 1)))) return rc;
        if ((rc = h->d_flip_i32.ensure((size_t)B * (T + 1)))) return rc;
        if ((rc = h->d_out.ensure((size_t)B * h->K))) return rc;
        if ((rc = h->d_bytes_b.ensure(2 * (size_t)B))) return rc;
        c.mag = h->d_list_out.p; c.flip = h->d_flip_i32.p; c.cand = c.flip + B; c.out = h->d_out.p; c.crc_ok = h->d_bytes_b.p; c.n_dec = c.crc_ok + B;
        return POLAR_OK;
    }
};

}  // namespace

extern "C" {

int polar_decode_sc_flip_batch_dev(polar_code_t *h, const void *d_llr, int fmt, long B, int max_flips, uint8_t *d_out, uint8_t *d_crc_ok,
                                   uint8_t *d_n_dec, int32_t *d_flip, int32_t *d_cand, double *d_mag, void *stream) {
    return on_device(h, flip_check(h, d_llr, fmt, B, max_flips, d_out), B, [&]() -> int {
        if (int rc = flip_prepare(h)) return rc;
        return flip_launch(h, d_llr, fmt, B, max_flips, d_out, d_crc_ok, d_n_dec, d_flip, d_cand, d_mag, (hipStream_t)stream);
    });
}

// One copy in, the launch, a wait, the copies out.
int polar_decode_sc_flip_batch(polar_code_t *h, const void *llr, int fmt, long B, int max_flips, uint8_t *out, uint8_t *crc_ok,
                               uint8_t *n_dec, int32_t *flip, int32_t *cand, double *mag) {
    return on_device(h, flip_check(h, llr, fmt, B, max_flips, out), B, [&]() -> int {
        int rc;
        if ((rc = flip_prepare(h))) return rc;
        if ((rc = stage_rows(h, llr, fmt, B))) return rc;
        FlipChunk d;
        if ((rc = FlipChunk::make(h, B, max_flips, d))) return rc;
        const size_t T = (size_t)max_flips;
        if ((rc = flip_launch(h, h->d_in.p, fmt, B, max_flips, d.out, crc_ok ? d.crc_ok : nullptr, n_dec ? d.n_dec : nullptr,
                              flip ? d.flip : nullptr, cand ? d.cand : nullptr, mag ? d.mag : nullptr, nullptr))) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        if ((rc = copy_back(out, 0, d.out, (size_t)B * h->K)) || (rc = copy_back(crc_ok, 0, d.crc_ok, (size_t)B)) ||
            (rc = copy_back(n_dec, 0, d.n_dec, (size_t)B)) || (rc = copy_back(flip, 0, d.flip, (size_t)B))) return rc;
        if (T && ((rc = copy_back(cand, 0, d.cand, (size_t)B * T)) || (rc = copy_back(mag, 0, d.mag, (size_t)B * T)))) return rc;
        return POLAR_OK;
    });
}

// Per enabled point and per chunk of trials, stream-ordered: the trials' LLRs and sent info (synth_kernel), the decode, the
// classification. The counters stay on the device until the end.
int polar_mc_batch_flip(polar_code_t *h, int constellation, uint64_t seed, uint64_t t0, long T, long stride, const double *axis, int n_e,
                        int max_flips, const uint8_t *enabled, uint64_t *stats) {
    Sweep sw;
    int rc = sweep_begin(sw, h, axis && enabled && stats, "SC-Flip decoder has", constellation, seed, t0, T, stride, axis, n_e > 0, stats,
                         [&]() -> int {
        if (int r = flip_check_code(h, max_flips)) return r;
        return flip_check_size(h);
    });
    if (rc || T == 0) return rc;
    const int N = h->N, K = h->K;
    const long chunk = sweep_chunk(h, T, (size_t)N * sizeof(double) + 2 * (size_t)K + 2);
    // (every buffer at its largest before the first launch)
    if ((rc = flip_prepare(h))) return rc;
    if ((rc = sweep_rows(h, chunk))) return rc;
    FlipChunk d;
    if ((rc = FlipChunk::make(h, chunk, 0, d))) return rc;
    const auto cells = sweep_cells(enabled, 1, n_e, POLAR_FL_N, {chunk});
    return sweep_walk(sw, cells, POLAR_FL_N, 1, n_e, [&](const SweepCell &cell, long c, const PolarEncodeParams &) -> int {
        if (int r = flip_launch(h, h->d_in.p, POLAR_LLR_F64, c, max_flips, d.out, d.crc_ok, d.n_dec, nullptr, nullptr, nullptr, nullptr)) return r;
        HIP_TRY(polar_launch_flip_classify(d.out, d.crc_ok, d.n_dec, h->d_bytes_a.p, c, K, h->d_mc_ctr.p + cell.ctr, nullptr));
        return POLAR_OK;
    });
}

}  // extern "C"
