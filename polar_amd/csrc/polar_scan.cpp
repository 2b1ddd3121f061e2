// polar_scan.cpp — SCAN soft-output decoding (include/polar_amd.h polar_decode_scan_batch*): the SC schedule with LLRs
// passed in both directions, a few iterations; per-bit LLRs of the info bits and extrinsic LLRs of the coded bits come out beside the
// hard word. One kernel (polar_kernels_scan.hip scan_kernel), one launch for the whole batch: the iterations and the early stop run in
// the kernel, the host chains nothing. The handle's mode, tuning and latency threshold are not looked at.
#include "polar_host.h"

namespace {

static_assert(POLAR_SCAN_MINSUM == POLAR_SCAN_F_MINSUM && POLAR_SCAN_EARLY_STOP == POLAR_SCAN_F_EARLY, "POLAR_SCAN_* flags");

// what the decode and the sweep refuse alike, after their pointers
int scan_check_code(const polar_code *h, int iters, int flags) {
    if (iters < 1 || iters > POLAR_SCAN_MAX_ITERS) return fail(POLAR_E_ARG, "iters %d out of range [1, %d]", iters, POLAR_SCAN_MAX_ITERS);
    if (flags & ~(POLAR_SCAN_MINSUM | POLAR_SCAN_EARLY_STOP)) return fail(POLAR_E_ARG, "unknown SCAN flag bits 0x%x", flags);
    if ((flags & POLAR_SCAN_EARLY_STOP) && h->crc == 0) return fail(POLAR_E_ARG, "SCAN early stop needs a CRC: this code has none to stop on");
    return POLAR_OK;
}
int scan_check_size(const polar_code *h) {
    return h->n > polar_scan_max_log() ? fail(POLAR_E_UNSUPPORTED, "SCAN keeps a codeword in LDS: n = %d is above %d", h->n, polar_scan_max_log()) : POLAR_OK;
}
int scan_check(const polar_code *h, const void *llr, int fmt, long B, int iters, int flags, const uint8_t *out) {
    if (!h || !llr || !out) return fail(POLAR_E_ARG, "NULL argument");
    if (int rc = scan_check_code(h, iters, flags)) return rc;
    if (int rc = llr_fmt_check(fmt, llr)) return rc;
    if (B < 0) return fail(POLAR_E_ARG, "negative batch");
    return scan_check_size(h);
}

// The walk of scan_kernel over the code tree, depth first; node v of layer lam covers the leaves [v << (n - lam), (v + 1) << (n - lam)).
// Nothing walks into an all-frozen subtree; an all-unfrozen one has no UP steps (its B is 0); a node of two leaves is ONE op. The root
// always gets its B: that is `ext`.
void scan_schedule(polar_code *h) {
    const int n = h->n;
    const LeafCount unf(h);
    auto kind = [&](int l, int w) {
        const int c = unf.under(l, w);
        return c == 0 ? POLAR_SCAN_KIND_FROZEN : c == (1 << (n - l)) ? POLAR_SCAN_KIND_UNFROZEN : POLAR_SCAN_KIND_MIXED;
    };
    auto emit = [&](int type, int lam, int v, int kl, int kr, int wb) {
        h->scan_ops.push_back((uint32_t)type | ((uint32_t)lam << 3) | ((uint32_t)v << 7) | ((uint32_t)kl << 23) | ((uint32_t)kr << 25) | ((uint32_t)wb << 27));
    };
    std::function<void(int, int)> go = [&](int lam, int v) {
        const int kl = kind(lam + 1, 2 * v), kr = kind(lam + 1, 2 * v + 1);
        const int wb = (kind(lam, v) == POLAR_SCAN_KIND_MIXED || lam == 0) ? 1 : 0;
        if (lam == n - 1) { emit(POLAR_SCAN_OP_PAIR, lam, v, kl, kr, wb); return; }
        if (kl != POLAR_SCAN_KIND_FROZEN) { emit(POLAR_SCAN_OP_LEFT, lam + 1, v, kl, kr, 0); go(lam + 1, 2 * v); }
        if (kr != POLAR_SCAN_KIND_FROZEN) { emit(POLAR_SCAN_OP_RIGHT, lam + 1, v, kl, kr, 0); go(lam + 1, 2 * v + 1); }
        if (wb) emit(POLAR_SCAN_OP_UP, lam, v, kl, kr, 1);
    };
    h->scan_ops.clear();
    go(0, 0);                                                                      // (K >= 1: the root is never all frozen)
}

int scan_prepare(polar_code *h) {
    return ops_prepare(h, polar_scan_lds_bytes(h->n), "the SCAN kernel's LDS does not fit this device", h->scan_ops, h->d_scan_ops, scan_schedule);
}

// (arguments checked, B > 0, the handle's device current, scan_prepare done)
int scan_launch(polar_code *h, const void *d_llr, int fmt, long B, int iters, int flags, uint8_t *d_out, double *d_info_llr, double *d_ext,
                uint8_t *d_crc_ok, uint8_t *d_n_iter, hipStream_t st) {
    PolarScanParams p;
    p.n = h->n; p.N = h->N; p.K = h->K; p.crc = h->crc; p.iters = iters; p.flags = flags; p.B = B;
    p.llr = d_llr; p.llr_fmt = fmt; p.ops = h->d_scan_ops.p; p.n_ops = (int)h->scan_ops.size();
    p.order = h->d_order.p; p.crcm = h->d_crcm.p; p.tabs = h->d_tabs.p;
    p.out = d_out; p.info_llr = d_info_llr; p.ext = d_ext; p.crc_ok = d_crc_ok; p.n_iter = d_n_iter;
    HIP_TRY(polar_launch_scan(p, (int)std::min<long>(B, polar_scan_grid_cap()), st));
    return POLAR_OK;
}

// One chunk of the host form's and the sweep's outputs: the soft values in d_list_out (info_llr, then ext; the sweep asks for
// neither), the words in d_out, crc_ok and n_iter in d_bytes_b
struct ScanChunk {
    double *info_llr, *ext; uint8_t *out, *crc_ok, *n_iter;
    static int make(polar_code *h, long B, bool soft, ScanChunk &c) {
        int rc;
        if ((rc = h->d_list_out.ensure(soft ? (size_t)B * (h->K + h->N) : 1))) return rc;
        if ((rc = h->d_out.ensure((size_t)B * h->K))) return rc;
        if ((rc = h->d_bytes_b.ensure(2 * (size_t)B))) return rc;
        c.info_llr = h->d_list_out.p; c.ext = c.info_llr + (size_t)B * h->K; c.out = h->d_out.p; c.crc_ok = h->d_bytes_b.p; c.n_iter = c.crc_ok + B;
        return POLAR_OK;
    }
};

}  // namespace

extern "C" {

int polar_decode_scan_batch_dev(polar_code_t *h, const void *d_llr, int fmt, long B, int iters, int flags, uint8_t *d_out,
                                double *d_info_llr, double *d_ext, uint8_t *d_crc_ok, uint8_t *d_n_iter, void *stream) {
    return on_device(h, scan_check(h, d_llr, fmt, B, iters, flags, d_out), B, [&]() -> int {
        if (int rc = scan_prepare(h)) return rc;
        return scan_launch(h, d_llr, fmt, B, iters, flags, d_out, d_info_llr, d_ext, d_crc_ok, d_n_iter, (hipStream_t)stream);
    });
}

// One copy in, the launch, a wait, the copies out.
int polar_decode_scan_batch(polar_code_t *h, const void *llr, int fmt, long B, int iters, int flags, uint8_t *out, double *info_llr,
                            double *ext, uint8_t *crc_ok, uint8_t *n_iter) {
    return on_device(h, scan_check(h, llr, fmt, B, iters, flags, out), B, [&]() -> int {
        int rc;
        if ((rc = scan_prepare(h))) return rc;
        if ((rc = stage_rows(h, llr, fmt, B))) return rc;
        ScanChunk d;
        if ((rc = ScanChunk::make(h, B, true, d))) return rc;
        if ((rc = scan_launch(h, h->d_in.p, fmt, B, iters, flags, d.out, info_llr ? d.info_llr : nullptr, ext ? d.ext : nullptr,
                              crc_ok ? d.crc_ok : nullptr, n_iter ? d.n_iter : nullptr, nullptr))) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        if ((rc = copy_back(out, 0, d.out, (size_t)B * h->K)) || (rc = copy_back(info_llr, 0, d.info_llr, (size_t)B * h->K)) ||
            (rc = copy_back(ext, 0, d.ext, (size_t)B * h->N)) || (rc = copy_back(crc_ok, 0, d.crc_ok, (size_t)B)) ||
            (rc = copy_back(n_iter, 0, d.n_iter, (size_t)B))) return rc;
        return POLAR_OK;
    });
}

// Per enabled point and per chunk of trials, stream-ordered: the trials' LLRs and sent info (synth_kernel), the decode, the
// classification. The counters stay on the device until the end.
int polar_mc_batch_scan(polar_code_t *h, int constellation, uint64_t seed, uint64_t t0, long T, long stride, const double *axis, int n_e,
                        int iters, int flags, const uint8_t *enabled, uint64_t *stats) {
    Sweep sw;
    int rc = sweep_begin(sw, h, axis && enabled && stats, "SCAN decoder has", constellation, seed, t0, T, stride, axis, n_e > 0, stats,
                         [&]() -> int {
        if (int r = scan_check_code(h, iters, flags)) return r;
        return scan_check_size(h);
    });
    if (rc || T == 0) return rc;
    const int N = h->N, K = h->K;
    const long chunk = sweep_chunk(h, T, (size_t)N * sizeof(double) + 2 * (size_t)K + 2);
    // (every buffer at its largest before the first launch)
    if ((rc = scan_prepare(h))) return rc;
    if ((rc = sweep_rows(h, chunk))) return rc;
    ScanChunk d;
    if ((rc = ScanChunk::make(h, chunk, false, d))) return rc;
    const auto cells = sweep_cells(enabled, 1, n_e, POLAR_SN_N, {chunk});
    return sweep_walk(sw, cells, POLAR_SN_N, 1, n_e, [&](const SweepCell &cell, long c, const PolarEncodeParams &) -> int {
        if (int r = scan_launch(h, h->d_in.p, POLAR_LLR_F64, c, iters, flags, d.out, nullptr, nullptr, d.crc_ok, d.n_iter, nullptr)) return r;
        HIP_TRY(polar_launch_scan_classify(d.out, d.crc_ok, d.n_iter, h->d_bytes_a.p, c, K, h->crc > 0, h->d_mc_ctr.p + cell.ctr, nullptr));
        return POLAR_OK;
    });
}

}  // extern "C"
