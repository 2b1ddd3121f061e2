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

}  // extern "C"
