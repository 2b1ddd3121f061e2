// polar_list.cpp — list output of decode_scl_llr: every path the list decoder holds at the end of a codeword, with its metric
// and CRC result (include/polar_amd.h polar_decode_scl_llr_list_batch*), and the search for a given word in it.
// One kernel family: the LLR-domain batch kernel with the list-output finish (polar_kernels.hip, POLAR_ED_TU = 4) at the default
// tuning — no exp-domain pass, so no fallback pass; no one-codeword-per-wave form; the handle's mode and tuning are not looked at.
#include "polar_host.h"

namespace {

int list_check(const polar_code *h, const void *llr, int fmt, long B, int L, const uint8_t *cand) {
    if (!h || !llr || !cand) return fail(POLAR_E_ARG, "NULL argument");
    int rc = llr_fmt_check(fmt, llr);
    if (rc) return rc;
    if (L < 1 || L > POLAR_MAX_LIST) return fail(POLAR_E_ARG, "list size %d out of range [1, %d]", L, POLAR_MAX_LIST);
    if (B < 0) return fail(POLAR_E_ARG, "negative batch");
    return POLAR_OK;
}

// (arguments checked, B > 0, the handle's device current)
int list_launch(polar_code *h, const void *d_llr, int fmt, long B, int L, uint8_t *d_cand, double *d_pm, uint8_t *d_crc_ok,
                int32_t *d_n_active, int32_t *d_winner, hipStream_t st) {
    const int gs = pow2ceil(L), G = 64 / gs;
    const int lds_log = 3, wpb = 4, wpc = 16;
    if (polar_decode_lds_bytes(lds_log, 0) > h->lds_per_block) return fail(POLAR_E_UNSUPPORTED, "the list kernel's LDS does not fit this device");
    const long groups = (B + G - 1) / G;
    int grid = (int)std::min<long>(groups, (long)h->num_cu * wpc);
    grid = ((grid + wpb - 1) / wpb) * wpb;          // whole blocks
    const int SL = 1 << lds_log;
    const size_t big = (h->N > 2 * SL) ? (size_t)(h->N - 2 * SL) : 0;
    const size_t cwords = (h->N >= 128) ? (size_t)(h->N / 32 - 2) : 0;
    int rc;
    // the per-wave state scratch (the decode's own buffers, grown on demand); a device too full for it runs fewer persistent waves
    for (;;) {
        rc = h->d_llr_scr.ensure((size_t)grid * big * 64 + 64);
        if (rc != POLAR_E_NOMEM || grid <= wpb) break;
        (void)hipGetLastError();
        grid = std::max(wpb, (grid / 2 / wpb) * wpb);
    }
    if (rc) return rc;
    if ((rc = h->d_c_scr.ensure((size_t)grid * 2 * cwords * 64 + 64))) return rc;
    if ((rc = h->d_hist_scr.ensure((size_t)grid * 3 * h->W * 64 + 64))) return rc;
    if ((rc = h->d_work.ensure(1))) return rc;
    PolarListParams p;
    p.n = h->n; p.N = h->N; p.K = h->K; p.crc = h->crc; p.L = L; p.W = h->W; p.B = B;
    prefix_geometry(h, gs, &p.prefix_q, &p.prefix_len);
    p.llr = (const double *)d_llr; p.llr_fmt = fmt; p.p0 = nullptr; p.out = nullptr; p.pm_out = nullptr;
    p.frozen = h->d_frozen.p; p.info_rank = h->d_info_rank.p; p.crc_mask = h->d_crc_mask.p; p.tabs = h->d_tabs.p;
    p.ctl = h->d_ctl.p;
    p.pre = nullptr;
    p.flags = nullptr; p.cw_list = nullptr; p.cw_count = nullptr; p.n_dev = nullptr;
    p.tab_scr = nullptr; p.var_scr = nullptr;
    if (p.prefix_q) {
        if ((rc = h->d_pre.ensure((size_t)B * (size_t)(h->N - p.prefix_q + 1)))) return rc;
        p.pre = h->d_pre.p;
    }
    p.llr_scr = h->d_llr_scr.p; p.c_scr = h->d_c_scr.p; p.hist_scr = h->d_hist_scr.p;
    p.work = h->d_work.p;
    p.list_cand = d_cand; p.list_pm = d_pm; p.list_crc = d_crc_ok; p.list_nact = d_n_active; p.list_win = d_winner;
    HIP_TRY(hipMemsetAsync(p.work, 0, sizeof(unsigned int), st));
    if (p.prefix_q) HIP_TRY(polar_launch_prefix(p, false, nullptr, st));
    HIP_TRY(polar_launch_decode_llr_list(p, gs, grid, st));
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
    if (!h || !d_cand || !d_n_active || !d_info || !d_rank) return fail(POLAR_E_ARG, "NULL argument");
    if (L < 1 || L > POLAR_MAX_LIST) return fail(POLAR_E_ARG, "list size %d out of range [1, %d]", L, POLAR_MAX_LIST);
    if (B <= 0) return B == 0 ? POLAR_OK : fail(POLAR_E_ARG, "negative batch");
    DevGuard dg_;
    int rc = ensure_device(h, dg_);
    if (rc) return rc;
    HIP_TRY(polar_launch_list_find(d_cand, d_n_active, d_info, B, L, h->K, d_rank, (hipStream_t)stream));
    return POLAR_OK;
}

}  // extern "C"
