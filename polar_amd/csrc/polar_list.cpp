// polar_list.cpp — list output of decode_scl_llr: every path the list decoder holds at the end of a codeword, with its metric
// and CRC result (include/polar_amd.h polar_decode_scl_llr_list_batch*), and the search for a given word in it.
// One kernel family: the LLR-domain batch kernel with the list-output finish (polar_kernels.hip, POLAR_ED_TU = 4) at the default
// tuning — no exp-domain pass, so no fallback pass; no one-codeword-per-wave form; the handle's mode and tuning are not looked at.
#include "polar_host.h"

namespace {

int list_check(const polar_code *h, const void *llr, int fmt, long B, int L, const uint8_t *cand) {
    return check_args(h && llr && cand, L, B, [&] { return llr_fmt_check(fmt, llr); });
}

// (arguments checked, B > 0, the handle's device current)
int list_launch(polar_code *h, const void *d_llr, int fmt, long B, int L, uint8_t *d_cand, double *d_pm, uint8_t *d_crc_ok,
                int32_t *d_n_active, int32_t *d_winner, hipStream_t st) {
    BatchGeometry g;
    if (!batch_geometry(h, B, L, false, g)) return fail(POLAR_E_UNSUPPORTED, "the list kernel's LDS does not fit this device");
    int rc;
    // the per-wave state scratch (the decode's own buffers, grown on demand); a device too full for it runs fewer persistent waves
    while ((rc = ensure_batch_scratch(h, g)) == POLAR_E_NOMEM && g.grid > g.wpb) {
        (void)hipGetLastError();
        g.grid = std::max(g.wpb, (g.grid / 2 / g.wpb) * g.wpb);
    }
    if (rc) return rc;
    if ((rc = h->d_work.ensure(1))) return rc;
    PolarListParams p;
    base_params(h, L, B, p);
    p.llr = (const double *)d_llr; p.llr_fmt = fmt;
    if ((rc = prefix_params(h, g.gs, p))) return rc;
    p.list_cand = d_cand; p.list_pm = d_pm; p.list_crc = d_crc_ok; p.list_nact = d_n_active; p.list_win = d_winner;
    HIP_TRY(hipMemsetAsync(p.work, 0, sizeof(unsigned int), st));
    if (p.prefix_q) HIP_TRY(polar_launch_prefix(p, false, nullptr, st));
    HIP_TRY(polar_launch_decode_llr_list(p, g.gs, g.grid, st));
    return POLAR_OK;
}

// ---- path metric of given words (polar_kernels_metric.hip) ----
int metric_check(const polar_code *h, const void *llr, int fmt, const uint8_t *info, long B, int R, const double *pm) {
    return check_args(h && llr && info && pm, R, B, [&] { return llr_fmt_check(fmt, llr); });
}

// (arguments checked, B > 0, the handle's device current) One wave per word; its N doubles in LDS while they fit, else in a row of
// the handle's scratch per resident wave
int metric_launch(polar_code *h, const void *d_llr, int fmt, const uint8_t *d_info, long B, int R, double *d_pm, hipStream_t st) {
    PolarMetricParams p;
    p.n = h->n; p.N = h->N; p.K = h->K; p.crc = h->crc; p.R = R; p.B = B;
    p.llr = d_llr; p.llr_fmt = fmt; p.info = d_info; p.order = h->d_order.p; p.crcm = h->d_crcm.p; p.tabs = h->d_tabs.p;
    p.scr = nullptr; p.pm = d_pm;
    const long words = B * (long)R;
    long grid = std::min<long>(words, 8192);
    if (polar_metric_lds_bytes(h->n, 1) > h->lds_per_block) {
        if (polar_metric_lds_bytes(h->n, 0) > h->lds_per_block) return fail(POLAR_E_UNSUPPORTED, "the path-metric kernel's LDS does not fit this device");
        grid = std::min<long>(grid, (long)h->num_cu * 2);
        int rc;
        if ((rc = h->d_metric_scr.ensure((size_t)grid * h->N))) return rc;
        p.scr = h->d_metric_scr.p;
    }
    HIP_TRY(polar_launch_path_metric(p, (int)grid, st));
    return POLAR_OK;
}

}  // namespace

extern "C" {

int polar_decode_scl_llr_list_batch_dev(polar_code_t *h, const void *d_llr, int fmt, long B, int L, uint8_t *d_cand, double *d_pm,
                                        uint8_t *d_crc_ok, int32_t *d_n_active, int32_t *d_winner, void *stream) {
    int rc = list_check(h, d_llr, fmt, B, L, d_cand);
    if (rc || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    return list_launch(h, d_llr, fmt, B, L, d_cand, d_pm, d_crc_ok, d_n_active, d_winner, (hipStream_t)stream);
}

// One copy in, then per chunk of codewords: the launches, a wait, the copies out. The chunk bounds the device memory the list
// takes (L K + 9 L + 8 bytes per codeword), not the input, which is resident for the whole call.
int polar_decode_scl_llr_list_batch(polar_code_t *h, const void *llr, int fmt, long B, int L, uint8_t *cand, double *pm,
                                    uint8_t *crc_ok, int32_t *n_active, int32_t *winner) {
    int rc = list_check(h, llr, fmt, B, L, cand);
    if (rc || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    const size_t esz = polar_llr_esz(fmt), row = (size_t)h->N * esz;
    if ((rc = h->d_in.ensure(((size_t)B * row + 7) / 8))) return rc;
    HIP_TRY(hipMemcpy(h->d_in.p, llr, (size_t)B * row, hipMemcpyHostToDevice));
    const size_t LK = (size_t)L * h->K, per = LK + 9 * (size_t)L + 8;
    const long chunk = std::min<long>(B, h->knobs.list_chunk_cw > 0 ? h->knobs.list_chunk_cw : std::max<long>(1, (long)(((size_t)256 << 20) / per)));
    // one buffer per chunk: metrics (doubles) first, then the two int32 arrays, then the bytes
    if ((rc = h->d_list_out.ensure(((size_t)chunk * per + 7) / 8 + 1))) return rc;
    double *d_pm = h->d_list_out.p;
    int32_t *d_na = reinterpret_cast<int32_t *>(d_pm + (size_t)chunk * L), *d_win = d_na + chunk;
    uint8_t *d_cand = reinterpret_cast<uint8_t *>(d_win + chunk), *d_crc = d_cand + (size_t)chunk * LK;
    for (long b0 = 0; b0 < B; b0 += chunk) {
        const long c = std::min(chunk, B - b0);
        if ((rc = list_launch(h, reinterpret_cast<const char *>(h->d_in.p) + (size_t)b0 * row, fmt, c, L, d_cand, pm ? d_pm : nullptr,
                              crc_ok ? d_crc : nullptr, n_active ? d_na : nullptr, winner ? d_win : nullptr, nullptr))) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        HIP_TRY(hipMemcpy(cand + (size_t)b0 * LK, d_cand, (size_t)c * LK, hipMemcpyDeviceToHost));
        if (pm) HIP_TRY(hipMemcpy(pm + (size_t)b0 * L, d_pm, (size_t)c * L * sizeof(double), hipMemcpyDeviceToHost));
        if (crc_ok) HIP_TRY(hipMemcpy(crc_ok + (size_t)b0 * L, d_crc, (size_t)c * L, hipMemcpyDeviceToHost));
        if (n_active) HIP_TRY(hipMemcpy(n_active + b0, d_na, (size_t)c * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (winner) HIP_TRY(hipMemcpy(winner + b0, d_win, (size_t)c * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return POLAR_OK;
}

int polar_list_find_dev(polar_code_t *h, const uint8_t *d_cand, const int32_t *d_n_active, const uint8_t *d_info, long B, int L,
                        int32_t *d_rank, void *stream) {
    int rc = check_args(h && d_cand && d_n_active && d_info && d_rank, L, B);
    if (rc || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    HIP_TRY(polar_launch_list_find(d_cand, d_n_active, d_info, B, L, h->K, d_rank, (hipStream_t)stream));
    return POLAR_OK;
}

int polar_path_metric_batch_dev(polar_code_t *h, const void *d_llr, int fmt, const uint8_t *d_info, long B, int R, double *d_pm, void *stream) {
    int rc = metric_check(h, d_llr, fmt, d_info, B, R, d_pm);
    if (rc || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    return metric_launch(h, d_llr, fmt, d_info, B, R, d_pm, (hipStream_t)stream);
}

int polar_path_metric_batch(polar_code_t *h, const void *llr, int fmt, const uint8_t *info, long B, int R, double *pm) {
    int rc = metric_check(h, llr, fmt, info, B, R, pm);
    if (rc || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    const size_t row = (size_t)h->N * polar_llr_esz(fmt), words = (size_t)B * R;
    if ((rc = h->d_in.ensure(((size_t)B * row + 7) / 8))) return rc;
    if ((rc = h->d_bytes_b.ensure(words * h->K))) return rc;
    if ((rc = h->d_list_out.ensure(words))) return rc;
    HIP_TRY(hipMemcpy(h->d_in.p, llr, (size_t)B * row, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_bytes_b.p, info, words * h->K, hipMemcpyHostToDevice));
    if ((rc = metric_launch(h, h->d_in.p, fmt, h->d_bytes_b.p, B, R, h->d_list_out.p, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(pm, h->d_list_out.p, words * sizeof(double), hipMemcpyDeviceToHost));
    return POLAR_OK;
}

// Per enabled (list size, point) and per chunk of trials, stream-ordered: the trials' LLRs and sent info (synth_kernel), the list
// decode, the sent word's own metric (one word per row), the classification. The counters stay on the device until the end.
int polar_mc_batch_list(polar_code_t *h, int constellation, uint64_t seed, uint64_t t0, long T, long stride, const double *axis, int n_e,
                        const uint8_t *L, int n_L, const uint8_t *enabled, uint64_t *stats) {
    if (!h || !axis || !L || !enabled || !stats) return fail(POLAR_E_ARG, "NULL argument");
    if (constellation & POLAR_RX_MLC) return fail(POLAR_E_ARG, "the list statistics have no MLC receiver");
    if (constellation != 0 && !is_ask_constellation(constellation)) return fail(POLAR_E_ARG, "unknown constellation %d", constellation);
    if (T < 0 || stride <= 0 || n_e <= 0 || n_L <= 0) return fail(POLAR_E_ARG, "bad sizes");
    for (int i = 0; i < n_L; ++i)
        if (L[i] < 1 || L[i] > POLAR_MAX_LIST) return fail(POLAR_E_ARG, "list size %d out of range", (int)L[i]);
    if (T == 0) return POLAR_OK;
    const int cid = constellation == POLAR_CONST_BPSK ? 0 : constellation;       // (BPSK on the Eb/N0 axis under either name)
    DevGuard dg_;
    int rc = ensure_device(h, dg_);
    if (rc) return rc;
    const int N = h->N, K = h->K, P = n_e * n_L;
    int Lmax = 1;
    for (int i = 0; i < n_L; ++i) Lmax = std::max<int>(Lmax, L[i]);
    auto chunk_of = [&](int Ls) {
        const size_t per = (size_t)Ls * K + 9 * (size_t)Ls + 8;
        return std::min<long>(T, h->knobs.list_chunk_cw > 0 ? h->knobs.list_chunk_cw : std::max<long>(1, (long)(((size_t)256 << 20) / per)));
    };
    long cmax = 0; size_t out_max = 0;
    for (int i = 0; i < n_L; ++i) {
        const long c = chunk_of(L[i]);
        cmax = std::max(cmax, c);
        out_max = std::max(out_max, (size_t)c * ((size_t)L[i] * K + 9 * (size_t)L[i] + 8));
    }
    // (every buffer at its largest before the first launch: a DevBuf that grows frees what work in flight may still read)
    if ((rc = h->d_in.ensure((size_t)cmax * N))) return rc;
    if ((rc = h->d_bytes_a.ensure((size_t)cmax * K))) return rc;                 // sent info
    if ((rc = h->d_list_out.ensure((out_max + 7) / 8 + 1 + (size_t)cmax))) return rc;
    if ((rc = h->d_mc_ctr.ensure((size_t)POLAR_LS_N * P))) return rc;
    HIP_TRY(hipMemsetAsync(h->d_mc_ctr.p, 0, (size_t)POLAR_LS_N * P * sizeof(unsigned long long), nullptr));
    for (int li = 0; li < n_L; ++li) {
        const int Ls = L[li];
        const long chunk = chunk_of(Ls);
        const size_t LK = (size_t)Ls * K;
        // one chunk of list output: metrics first, the sent words' metrics, the two int32 arrays, then the bytes
        double *d_pm = h->d_list_out.p, *d_pms = d_pm + (size_t)chunk * Ls;
        int32_t *d_na = reinterpret_cast<int32_t *>(d_pms + chunk), *d_win = d_na + chunk;
        uint8_t *d_cand = reinterpret_cast<uint8_t *>(d_win + chunk), *d_crc = d_cand + (size_t)chunk * LK;
        for (int ie = 0; ie < n_e; ++ie) {
            if (!enabled[li * n_e + ie]) continue;
            for (long c0 = 0; c0 < T; c0 += chunk) {
                const long c = std::min(chunk, T - c0);
                PolarEncodeParams p;
                fill_enc(h, p);
                p.B = c; p.seed = seed; p.trial0 = t0 + (uint64_t)c0 * (uint64_t)stride; p.stride = stride;
                fill_channel(h, p, cid, axis[ie]);
                p.llr = h->d_in.p; p.info_out = h->d_bytes_a.p;
                HIP_TRY(polar_launch_synth(p, nullptr));
                if ((rc = list_launch(h, h->d_in.p, POLAR_LLR_F64, c, Ls, d_cand, d_pm, d_crc, d_na, d_win, nullptr))) return rc;
                if ((rc = metric_launch(h, h->d_in.p, POLAR_LLR_F64, h->d_bytes_a.p, c, 1, d_pms, nullptr))) return rc;
                HIP_TRY(polar_launch_list_classify(d_cand, d_pm, d_crc, d_na, d_win, h->d_bytes_a.p, d_pms, c, Ls, K, nullptr,
                                                   h->d_mc_ctr.p + (size_t)POLAR_LS_N * (li * n_e + ie), nullptr));
            }
        }
    }
    std::vector<unsigned long long> ctr((size_t)POLAR_LS_N * P);
    HIP_TRY(hipMemcpy(ctr.data(), h->d_mc_ctr.p, ctr.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int i = 0; i < P; ++i)
        if (enabled[i])
            for (int k = 0; k < POLAR_LS_N; ++k) stats[(size_t)i * POLAR_LS_N + k] += (uint64_t)ctr[(size_t)i * POLAR_LS_N + k];
    return POLAR_OK;
}

}  // extern "C"
