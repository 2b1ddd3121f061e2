// polar_rm.cpp — rate matching (include/polar_amd.h polar_rm_pattern ... polar_ga_construction_init): the built-in
// patterns and the forced-frozen leaves (host only, no handle), the pattern of a handle with its checks and its inverse tables, the
// entry points around polar_kernels_rm.hip, the rate-matched workload and its sweep, the construction from a start vector.
// No decoder changes: a rate-matched receiver is the recover kernel followed by decode_impl.
#include "polar_host.h"
#include "polar_rm.h"
#include "polar_sys.h"

struct RmTables {
    int E = 0, max_src = 0;
    bool plain = true;                                 // neither punctured nor known positions: pure repetition (or the identity)
    double short_llr = 0.0;
    std::vector<uint16_t> sel;                         // [E]
    std::vector<uint8_t> known;                        // [N]
    std::vector<uint32_t> desc, src;                   // the inverse (polar_rm.h): [N][2], [E]
    DevBuf<uint16_t> d_sel;
    DevBuf<uint32_t> d_desc, d_src;
    bool uploaded = false;
    // scratch: the recovered rows of the decode; coded / transmit bits and received rows of the workload; staging of the host forms
    DevBuf<double> d_llr, d_rx;
    DevBuf<uint8_t> d_coded, d_tx, d_stage;
};

namespace {

const int kP32[32] = {0, 1, 2, 4, 3, 5, 6, 7, 8, 16, 9, 17, 10, 18, 11, 19, 12, 20, 13, 21, 14, 22, 15, 23, 24, 25, 26, 28, 27, 29, 30, 31};

inline int bitrev_n(int i, int n) {
    int r = 0;
    for (int k = 0; k < n; ++k) r |= ((i >> k) & 1) << (n - 1 - k);
    return r;
}

int pattern_check(int n, const uint16_t *sel, int E) {
    if (n < 1 || n > POLAR_MAX_N_LOG2) return fail(POLAR_E_ARG, "n = %d out of range [1, %d]", n, POLAR_MAX_N_LOG2);
    const int N = 1 << n;
    if (E < 1 || E > 8 * N) return fail(POLAR_E_ARG, "E = %d out of range [1, %d]", E, 8 * N);
    if (!sel) return fail(POLAR_E_ARG, "NULL argument");
    for (int e = 0; e < E; ++e)
        if (sel[e] >= N) return fail(POLAR_E_ARG, "sel[%d] = %d is not below N = %d", e, (int)sel[e], N);
    return POLAR_OK;
}

// the leaves a design must freeze (include/polar_amd.h "forced"); sent[p] = how often coded position p is transmitted
void forced_leaves(int n, const std::vector<uint32_t> &sent, const uint8_t *known, std::vector<uint8_t> &forced) {
    const int N = 1 << n;
    forced.assign(N, 0);
    if (known)
        for (int p = 0; p < N; ++p) {
            if (!known[p]) continue;
            const int j = bitrev_n(p, n);
            // (the leaves b with b & j == j: j with every subset of its clear bits)
            const int free_bits = (N - 1) & ~j;
            for (int s = free_bits;; s = (s - 1) & free_bits) {
                forced[j | s] = 1;
                if (!s) break;
            }
        }
    std::vector<uint8_t> a(N), b(N);
    for (int p = 0; p < N; ++p) a[p] = !sent[p] && !(known && known[p]);
    for (int st = 0; st < n; ++st) {
        for (int q = 0; q < N / 2; ++q) {
            const uint8_t c1 = a[2 * q], c2 = a[2 * q + 1];
            b[q] = c1 | c2;
            b[N / 2 + q] = c1 & c2;
        }
        a.swap(b);
    }
    for (int i = 0; i < N; ++i)
        if (a[bitrev_n(i, n)]) forced[i] = 1;
}

int rm_need(const polar_code *h) { return h->rm ? POLAR_OK : fail(POLAR_E_ARG, "no rate-matching pattern set (polar_set_rate_match)"); }

// tables on the device, BEFORE a launch (the handle's device current)
int rm_prepare(polar_code *h) {
    RmTables &t = *h->rm;
    if (t.uploaded) return POLAR_OK;
    int rc;
    if ((rc = upload(t.d_sel, t.sel)) || (rc = upload(t.d_desc, t.desc)) || (rc = upload(t.d_src, t.src))) return rc;
    t.uploaded = true;
    return POLAR_OK;
}

int recover_launch(polar_code *h, const void *d_rx, int fmt, long B, double *d_llr, hipStream_t st) {
    const RmTables &t = *h->rm;
    PolarRmParams p;
    p.N = h->N; p.E = t.E; p.B = B; p.desc = t.d_desc.p; p.src = t.d_src.p; p.max_src = t.max_src; p.short_llr = t.short_llr;
    HIP_TRY(polar_launch_rm_recover(p, d_rx, fmt, d_llr, st));
    return POLAR_OK;
}

// The dispatch rule: a pattern with punctured or known positions decodes in the LLR-domain family for this call — the effective mode
// of the handle is overridden while the scope lives and restored on every exit path
struct LlrFamilyScope {
    polar_code *h;
    int saved;
    LlrFamilyScope(polar_code *h_, bool force) : h(h_), saved(h_->knobs.mode_override) { if (force) h->knobs.mode_override = 1; }
    ~LlrFamilyScope() { h->knobs.mode_override = saved; }
};
int decode_recovered(polar_code *h, const double *d_llr, long B, int L, uint8_t *d_out, double *d_pm, hipStream_t st) {
    LlrFamilyScope scope(h, !h->rm->plain);
    return decode_impl(h, d_llr, POLAR_LLR_F64, B, nullptr, L, d_out, d_pm, st, nullptr, nullptr);
}

// the trials' info bits into d_info, their transmit bits' LLR rows into d_rx (buffers sized by the caller, rm_prepare done)
int synth_launch(polar_code *h, uint64_t seed, uint64_t trial0, long stride, long B, double s, double *d_rx, uint8_t *d_info, bool draw,
                 hipStream_t st) {
    RmTables &t = *h->rm;
    PolarEncodeParams p;
    fill_enc(h, p);
    p.B = B; p.seed = seed; p.trial0 = trial0; p.stride = stride;
    p.info_out = d_info;
    if (draw) HIP_TRY(polar_launch_sys_draw(p, st));
    p.info = d_info; p.coded = t.d_coded.p;
    HIP_TRY(polar_launch_encode(p, st));
    HIP_TRY(polar_launch_rm_select(t.d_coded.p, t.d_sel.p, B, h->N, t.E, t.d_tx.p, st));
    HIP_TRY(polar_launch_rm_channel(t.d_tx.p, B, t.E, seed, trial0, stride, s, d_rx, st));
    return POLAR_OK;
}

}  // namespace

void polar_host::rm_release(polar_code *h) {
    if (!h->rm) return;
    RmTables *t = h->rm;
    t->d_sel.release(); t->d_desc.release(); t->d_src.release();
    t->d_llr.release(); t->d_rx.release(); t->d_coded.release(); t->d_tx.release(); t->d_stage.release();
    delete t;
    h->rm = nullptr;
}

extern "C" {

int polar_rm_pattern(int n, int E, int scheme, int Kp, uint16_t *sel, uint8_t *known) {
    if (n < 1 || n > POLAR_MAX_N_LOG2) return fail(POLAR_E_ARG, "n = %d out of range [1, %d]", n, POLAR_MAX_N_LOG2);
    const int N = 1 << n;
    if (E < 1 || E > 8 * N) return fail(POLAR_E_ARG, "E = %d out of range [1, %d]", E, 8 * N);
    if (!sel) return fail(POLAR_E_ARG, "NULL argument");
    if (known) memset(known, 0, N);
    switch (scheme) {
        case POLAR_RM_PUNCTURE:
            if (E >= N) return fail(POLAR_E_ARG, "puncturing needs E < N (E = %d, N = %d)", E, N);
            for (int e = 0; e < E; ++e) sel[e] = (uint16_t)(N - E + e);
            return POLAR_OK;
        case POLAR_RM_SHORTEN:
            if (E >= N) return fail(POLAR_E_ARG, "shortening needs E < N (E = %d, N = %d)", E, N);
            if (!known) return fail(POLAR_E_ARG, "NULL known");
            for (int e = 0; e < E; ++e) sel[e] = (uint16_t)e;
            for (int p = E; p < N; ++p) known[p] = 1;
            return POLAR_OK;
        case POLAR_RM_REPEAT:
            if (E < N) return fail(POLAR_E_ARG, "repetition needs E >= N (E = %d, N = %d)", E, N);
            for (int e = 0; e < E; ++e) sel[e] = (uint16_t)(e % N);
            return POLAR_OK;
        case POLAR_RM_NR: {
            if (n < 5) return fail(POLAR_E_ARG, "the NR pattern needs n >= 5");
            std::vector<uint16_t> y(N);
            for (int j = 0; j < N; ++j) y[j] = (uint16_t)bitrev_n(kP32[32 * j / N] * (N / 32) + j % (N / 32), n);
            if (E >= N) {
                for (int e = 0; e < E; ++e) sel[e] = y[e % N];
            } else if (16 * (long)Kp <= 7 * (long)E) {
                for (int e = 0; e < E; ++e) sel[e] = y[e + N - E];
            } else {
                if (!known) return fail(POLAR_E_ARG, "NULL known");
                for (int e = 0; e < E; ++e) sel[e] = y[e];
                for (int j = E; j < N; ++j) known[y[j]] = 1;
            }
            return POLAR_OK;
        }
    }
    return fail(POLAR_E_ARG, "unknown rate-matching scheme %d", scheme);
}

int polar_rm_forced(int n, const uint16_t *sel, int E, const uint8_t *known, uint8_t *forced) {
    if (int rc = pattern_check(n, sel, E)) return rc;
    if (!forced) return fail(POLAR_E_ARG, "NULL argument");
    const int N = 1 << n;
    std::vector<uint32_t> sent(N, 0);
    for (int e = 0; e < E; ++e) ++sent[sel[e]];
    std::vector<uint8_t> f;
    forced_leaves(n, sent, known, f);
    memcpy(forced, f.data(), N);
    return (int)std::count(f.begin(), f.end(), (uint8_t)1);
}

int polar_set_rate_match(polar_code_t *h, const uint16_t *sel, int E, const uint8_t *known, double short_llr) {
    if (!h) return fail(POLAR_E_ARG, "NULL handle");
    if (E == 0) {
        DevGuard dg;
        if (h->rm && h->dev_ready) { int rc = ensure_device(h, dg); if (rc) return rc; }
        rm_release(h);
        return POLAR_OK;
    }
    if (int rc = pattern_check(h->n, sel, E)) return rc;
    if (!(std::isfinite(short_llr) && short_llr > 0)) return fail(POLAR_E_ARG, "short_llr = %g is not finite and positive", short_llr);
    const int N = h->N, n = h->n;
    std::vector<uint32_t> sent(N, 0);
    for (int e = 0; e < E; ++e) ++sent[sel[e]];
    bool plain = true;
    for (int p = 0; p < N; ++p) {
        if (known && known[p] && sent[p]) return fail(POLAR_E_ARG, "coded position %d is known and also sent", p);
        if (!sent[p]) plain = false;
    }
    if (known)
        for (int p = 0; p < N; ++p) {
            if (!known[p]) continue;
            const int j = bitrev_n(p, n);
            for (int b = j; b < N; ++b)
                if ((b & j) == j && !h->frozen[b])
                    return fail(POLAR_E_ARG, "leaf %d is unfrozen, but coded position %d is known: the word is not 0 there", b, p);
        }
    auto tp = std::make_unique<RmTables>();
    RmTables &t = *tp;
    t.E = E; t.short_llr = short_llr; t.plain = plain;
    t.sel.assign(sel, sel + E);
    t.known.assign(N, 0);
    if (known) for (int p = 0; p < N; ++p) t.known[p] = known[p] ? 1 : 0;
    // the inverse: per coded position its sources in ascending e
    std::vector<uint32_t> off(N + 1, 0);
    for (int p = 0; p < N; ++p) off[p + 1] = off[p] + sent[p];
    t.src.assign(E, 0);
    std::vector<uint32_t> fill(off.begin(), off.end() - 1);
    for (int e = 0; e < E; ++e) t.src[fill[sel[e]]++] = (uint32_t)e;
    t.desc.assign((size_t)2 * N, 0);
    for (int p = 0; p < N; ++p) {
        t.desc[2 * p] = sent[p] | (t.known[p] ? kRmKnown : 0u);
        t.desc[2 * p + 1] = sent[p] == 1 ? t.src[off[p]] : off[p];
        t.max_src = std::max(t.max_src, (int)sent[p]);
    }
    {
        DevGuard dg;
        if (h->rm && h->dev_ready) { int rc = ensure_device(h, dg); if (rc) return rc; }
        rm_release(h);
    }
    h->rm = tp.release();
    return POLAR_OK;
}

int polar_get_rate_match(const polar_code_t *h, int *E, uint16_t *sel, uint8_t *known, double *short_llr) {
    if (!h) return fail(POLAR_E_ARG, "NULL handle");
    if (E) *E = h->rm ? h->rm->E : 0;
    if (!h->rm) return POLAR_OK;
    if (sel) memcpy(sel, h->rm->sel.data(), 2 * (size_t)h->rm->E);
    if (known) memcpy(known, h->rm->known.data(), h->N);
    if (short_llr) *short_llr = h->rm->short_llr;
    return POLAR_OK;
}

double polar_snr_sqrt_linear_rm(const polar_code_t *h, double ebno_db) {   // polar_snr_sqrt_linear (PolarCode.cpp:744-745) at rate K / E
    if (!h || !h->rm) return NAN;
    return std::pow(10.0f, ebno_db / 20) * std::sqrt(((double)h->K) / ((double)h->rm->E));
}

int polar_rate_match_batch_dev(polar_code_t *h, const uint8_t *d_coded, long B, uint8_t *d_tx, void *stream) {
    return on_device(h, check_args(h && d_coded && d_tx, kNoList, B, [&] { return rm_need(h); }), B, [&]() -> int {
        if (int rc = rm_prepare(h)) return rc;
        HIP_TRY(polar_launch_rm_select(d_coded, h->rm->d_sel.p, B, h->N, h->rm->E, d_tx, (hipStream_t)stream));
        return POLAR_OK;
    });
}
int polar_rate_match_batch(polar_code_t *h, const uint8_t *coded, long B, uint8_t *tx) {
    return on_device(h, check_args(h && coded && tx, kNoList, B, [&] { return rm_need(h); }), B, [&]() -> int {
        int rc;
        if ((rc = rm_prepare(h))) return rc;
        RmTables &t = *h->rm;
        if ((rc = t.d_coded.ensure((size_t)B * h->N)) || (rc = t.d_tx.ensure((size_t)B * t.E))) return rc;
        HIP_TRY(hipMemcpy(t.d_coded.p, coded, (size_t)B * h->N, hipMemcpyHostToDevice));
        HIP_TRY(polar_launch_rm_select(t.d_coded.p, t.d_sel.p, B, h->N, t.E, t.d_tx.p, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        return copy_back(tx, 0, t.d_tx.p, (size_t)B * t.E);
    });
}

int polar_rate_recover_batch_dev(polar_code_t *h, const void *d_rx, int fmt, long B, double *d_llr, void *stream) {
    return on_device(h, check_args(h && d_rx && d_llr, kNoList, B, [&] { if (int rc = rm_need(h)) return rc; return llr_fmt_check(fmt, d_rx); }), B,
                     [&]() -> int {
        if (int rc = rm_prepare(h)) return rc;
        return recover_launch(h, d_rx, fmt, B, d_llr, (hipStream_t)stream);
    });
}
int polar_rate_recover_batch(polar_code_t *h, const void *rx, int fmt, long B, double *llr) {
    return on_device(h, check_args(h && rx && llr, kNoList, B, [&] { if (int rc = rm_need(h)) return rc; return llr_fmt_check(fmt, rx); }), B,
                     [&]() -> int {
        int rc;
        if ((rc = rm_prepare(h))) return rc;
        RmTables &t = *h->rm;
        const size_t bytes = (size_t)B * t.E * polar_llr_esz(fmt);
        if ((rc = t.d_stage.ensure(bytes)) || (rc = t.d_llr.ensure((size_t)B * h->N))) return rc;
        HIP_TRY(hipMemcpy(t.d_stage.p, rx, bytes, hipMemcpyHostToDevice));
        if ((rc = recover_launch(h, t.d_stage.p, fmt, B, t.d_llr.p, nullptr))) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        return copy_back(llr, 0, t.d_llr.p, (size_t)B * h->N);
    });
}

int polar_decode_scl_llr_rm_batch_dev(polar_code_t *h, const void *d_rx, int fmt, long B, int L, uint8_t *d_out, double *d_pm, void *stream) {
    return on_device(h, check_args(h && d_rx && d_out, L, B, [&] { if (int rc = rm_need(h)) return rc; return llr_fmt_check(fmt, d_rx); }), B,
                     [&]() -> int {
        int rc;
        if ((rc = rm_prepare(h))) return rc;
        RmTables &t = *h->rm;
        if ((rc = t.d_llr.ensure((size_t)B * h->N))) return rc;
        if ((rc = recover_launch(h, d_rx, fmt, B, t.d_llr.p, (hipStream_t)stream))) return rc;
        return decode_recovered(h, t.d_llr.p, B, L, d_out, d_pm, (hipStream_t)stream);
    });
}
int polar_decode_scl_llr_rm_batch(polar_code_t *h, const void *rx, int fmt, long B, int L, uint8_t *out) {
    return on_device(h, check_args(h && rx && out, L, B, [&] { if (int rc = rm_need(h)) return rc; return llr_fmt_check(fmt, rx); }), B,
                     [&]() -> int {
        int rc;
        if ((rc = rm_prepare(h))) return rc;
        RmTables &t = *h->rm;
        const size_t bytes = (size_t)B * t.E * polar_llr_esz(fmt);
        if ((rc = t.d_stage.ensure(bytes)) || (rc = t.d_llr.ensure((size_t)B * h->N)) || (rc = h->d_out.ensure((size_t)B * h->K))) return rc;
        HIP_TRY(hipMemcpy(t.d_stage.p, rx, bytes, hipMemcpyHostToDevice));
        if ((rc = recover_launch(h, t.d_stage.p, fmt, B, t.d_llr.p, nullptr))) return rc;
        if ((rc = decode_recovered(h, t.d_llr.p, B, L, h->d_out.p, nullptr, nullptr))) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        return copy_back(out, 0, h->d_out.p, (size_t)B * h->K);
    });
}

int polar_synth_rm_llr_dev(polar_code_t *h, uint64_t seed, uint64_t trial0, long B, double s, double *d_rx, uint8_t *d_info, void *stream) {
    return on_device(h, check_args(h && d_rx, kNoList, B, [&] { return rm_need(h); }), B, [&]() -> int {
        int rc;
        if ((rc = rm_prepare(h))) return rc;
        RmTables &t = *h->rm;
        if ((rc = t.d_coded.ensure((size_t)B * h->N)) || (rc = t.d_tx.ensure((size_t)B * t.E))) return rc;
        if (!d_info) { if ((rc = h->d_bytes_a.ensure((size_t)B * h->K))) return rc; d_info = h->d_bytes_a.p; }
        return synth_launch(h, seed, trial0, 1, B, s, d_rx, d_info, true, (hipStream_t)stream);
    });
}

// Per enabled (list size, point) and per chunk of trials, stream-ordered: the shared walk draws the trials' info bits; the encoder,
// the selection, the channel over the transmit bits at the rate K / E, the recover kernel (the walk's own LLR rows are replaced),
// decode_scl_llr under the dispatch rule, the classification. The counters stay on the device until the end.
int polar_mc_batch_rm(polar_code_t *h, uint64_t seed, uint64_t t0, long T, long stride, const double *ebno, int n_e, const uint8_t *L, int n_L,
                      const uint8_t *enabled, uint64_t *stats) {
    Sweep sw;
    int rc = sweep_begin(sw, h, ebno && L && enabled && stats, "rate-matched sweep has", 0, seed, t0, T, stride, ebno, n_e > 0 && n_L > 0, stats,
                         [&]() -> int { if (int r = rm_need(h)) return r; return check_list_sizes(L, n_L); });
    if (rc || T == 0) return rc;
    const int N = h->N, K = h->K, E = h->rm->E;
    const long chunk = sweep_chunk(h, T, (size_t)N * sizeof(double) + (size_t)N + (size_t)E * (1 + sizeof(double)) + 2 * (size_t)K);
    if ((rc = rm_prepare(h))) return rc;
    RmTables &t = *h->rm;
    if ((rc = sweep_rows(h, chunk)) || (rc = h->d_out.ensure((size_t)chunk * K)) || (rc = t.d_coded.ensure((size_t)chunk * N)) ||
        (rc = t.d_tx.ensure((size_t)chunk * E)) || (rc = t.d_rx.ensure((size_t)chunk * E))) return rc;
    const auto cells = sweep_cells(enabled, n_L, n_e, POLAR_RM_N, std::vector<long>(n_L, chunk));
    return sweep_walk(sw, cells, POLAR_RM_N, n_L, n_e, [&](const SweepCell &cell, long c, const PolarEncodeParams &p) -> int {
        const double s = polar_snr_sqrt_linear_rm(h, ebno[cell.point]);
        if (int r = synth_launch(h, p.seed, p.trial0, p.stride, c, s, t.d_rx.p, h->d_bytes_a.p, false, nullptr)) return r;
        if (int r = recover_launch(h, t.d_rx.p, POLAR_LLR_F64, c, h->d_in.p, nullptr)) return r;
        if (int r = decode_recovered(h, h->d_in.p, c, L[cell.row], h->d_out.p, nullptr, nullptr)) return r;
        HIP_TRY(polar_launch_rm_classify(h->d_out.p, h->d_bytes_a.p, c, K, h->d_mc_ctr.p + cell.ctr, nullptr));
        return POLAR_OK;
    });
}

int polar_ga_construction_init(int n, const double *init, const uint8_t *forced, int n_points, double phi_dx, double *channels,
                               uint16_t *order, double *bler_prefix) {
    if (n < 1 || n > POLAR_MAX_N_LOG2) return fail(POLAR_E_ARG, "n = %d out of range [1, %d]", n, POLAR_MAX_N_LOG2);
    if (n_points < 0 || (n_points && !init)) return fail(POLAR_E_ARG, "NULL argument or negative count");
    if (!(phi_dx >= 1e-7 && phi_dx <= 1.0)) return fail(POLAR_E_ARG, "phi_dx = %g out of range [1e-7, 1]", phi_dx);
    if (n_points == 0) return POLAR_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(POLAR_E_DEVICE, "no HIP device: the GA construction has no CPU path");
    const int N = 1 << n;
    const size_t tot = (size_t)n_points * N;
    DevBuf<double> d_f, d_init, d_scr, d_ch, d_pre;
    DevBuf<unsigned long long> d_i;
    DevBuf<uint16_t> d_ord;
    DevBuf<uint8_t> d_forced;
    struct Guard {
        DevBuf<double> &a, &b, &c, &d, &e; DevBuf<unsigned long long> &f; DevBuf<uint16_t> &g; DevBuf<uint8_t> &k;
        ~Guard() { a.release(); b.release(); c.release(); d.release(); e.release(); f.release(); g.release(); k.release(); }
    } guard{d_f, d_init, d_scr, d_ch, d_pre, d_i, d_ord, d_forced};
    int rc;
    if ((rc = d_f.ensure(POLAR_GA_PHI_FWD)) || (rc = d_i.ensure(POLAR_GA_PHI_INV)) || (rc = d_init.ensure(tot)) || (rc = d_scr.ensure(2 * tot)) ||
        (rc = d_ch.ensure(tot)) || (rc = d_pre.ensure(tot)) || (rc = d_ord.ensure(tot)) || (forced && (rc = d_forced.ensure(N)))) return rc;
    HIP_TRY(hipMemset(d_i.p, 0, POLAR_GA_PHI_INV * sizeof(unsigned long long)));
    HIP_TRY(polar_launch_ga_phi(d_f.p, d_i.p, phi_dx, (long)std::floor(400 / phi_dx + 1e-6) + 1, nullptr));
    HIP_TRY(hipMemcpy(d_init.p, init, tot * sizeof(double), hipMemcpyHostToDevice));
    if (forced) HIP_TRY(hipMemcpy(d_forced.p, forced, N, hipMemcpyHostToDevice));
    PolarRmGaParams p;
    p.n = n; p.N = N; p.init = d_init.p; p.forced = forced ? d_forced.p : nullptr; p.fwd = d_f.p; p.inv = d_i.p; p.scr = d_scr.p;
    p.channels = d_ch.p; p.order = d_ord.p; p.prefix = d_pre.p;
    HIP_TRY(polar_launch_rm_ga_construct(p, n_points, nullptr));
    if (channels) HIP_TRY(hipMemcpy(channels, d_ch.p, tot * sizeof(double), hipMemcpyDeviceToHost));
    if (order) HIP_TRY(hipMemcpy(order, d_ord.p, tot * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (bler_prefix) HIP_TRY(hipMemcpy(bler_prefix, d_pre.p, tot * sizeof(double), hipMemcpyDeviceToHost));
    if (!channels && !order && !bler_prefix) HIP_TRY(hipDeviceSynchronize());
    return POLAR_OK;
}

}  // extern "C"
