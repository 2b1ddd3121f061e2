// polar_adaptive.cpp — adaptive list decoding (include/polar_amd.h polar_decode_scl_llr_adaptive_batch*): a schedule of
// list sizes; a codeword is decoded with the next size only while its winner does not pass the CRC (Li, Shen, Tse 2012). One kernel
// family: the LLR-domain batch kernel with the adaptive finish (polar_kernels.hip, POLAR_ED_TU = 7) at the default tuning, as the list
// output — the handle's mode and tuning are not looked at. Stage 0 decodes the rows 0 .. B-1, every later stage a device-side work
// list that ed_collect_kernel builds from the retry bytes of the stage before; the host never learns a count.
#include "polar_host.h"

namespace {

// the handle's control block: work counter of stage s at [s], length of the work list stage s leaves at [kCtlCount + s]
constexpr int kCtlCount = POLAR_AD_MAX_STAGES, kCtlWords = 2 * POLAR_AD_MAX_STAGES;

int schedule_check(const uint8_t *Ls, int n_s) {
    if (n_s < 1 || n_s > POLAR_AD_MAX_STAGES) return fail(POLAR_E_ARG, "%d stages out of range [1, %d]", n_s, POLAR_AD_MAX_STAGES);
    for (int s = 0; s < n_s; ++s) {
        if (Ls[s] < 1 || Ls[s] > POLAR_MAX_LIST) return fail(POLAR_E_ARG, "list size %d out of range [1, %d]", (int)Ls[s], POLAR_MAX_LIST);
        if (s && Ls[s] <= Ls[s - 1]) return fail(POLAR_E_ARG, "the schedule is not strictly increasing at stage %d", s);
    }
    return POLAR_OK;
}

int adaptive_check(const polar_code *h, const void *llr, int fmt, long B, const uint8_t *Ls, int n_s, const uint8_t *out) {
    if (!h || !llr || !out || !Ls) return fail(POLAR_E_ARG, "NULL argument");
    if (int rc = schedule_check(Ls, n_s)) return rc;
    if (int rc = llr_fmt_check(fmt, llr)) return rc;
    if (B < 0) return fail(POLAR_E_ARG, "negative batch");
    if (h->crc == 0) return fail(POLAR_E_ARG, "adaptive decoding needs a CRC: this code has none to accept a word on");
    return POLAR_OK;
}

// the geometry of every stage of a call of B rows, and every buffer the launches use at its size — all of it BEFORE the first
// launch: a DevBuf that grows frees what work in flight may still read
int adaptive_prepare(polar_code *h, long B, const uint8_t *Ls, int n_s, BatchGeometry *g) {
    // (the grid of a later stage is sized for B as well: the host does not know how many codewords reach it; waves past the end
    // of the work list leave at once)
    for (int s = 0; s < n_s; ++s)
        if (!batch_geometry(h, B, Ls[s], false, g[s])) return fail(POLAR_E_UNSUPPORTED, "the list kernel's LDS does not fit this device");
    int rc;
    if ((rc = default_scratch(h, g, n_s))) return rc;                              // (the stages are sequential and share it)
    if ((rc = h->d_flags.ensure((size_t)B))) return rc;                            // retry bytes
    if ((rc = h->d_list.ensure((size_t)B))) return rc;                             // work list
    PolarDecodeParams pp;                                                          // stage 0's prefix buffer
    base_params(h, Ls[0], B, pp);
    if ((rc = prefix_params(h, g[0].gs, pp))) return rc;
    return h->d_adapt_ctl.ensure(kCtlWords);
}

// (arguments checked, B > 0, the handle's device current)
int adaptive_launch(polar_code *h, const void *d_llr, int fmt, long B, const uint8_t *Ls, int n_s, uint8_t *d_out, double *d_pm,
                    uint8_t *d_stage, uint8_t *d_crc_ok, hipStream_t st) {
    BatchGeometry g[POLAR_AD_MAX_STAGES];
    int rc;
    if ((rc = adaptive_prepare(h, B, Ls, n_s, g))) return rc;
    PolarAdaptParams p;
    base_params(h, Ls[0], B, p);
    p.llr = (const double *)d_llr; p.llr_fmt = fmt; p.out = d_out; p.pm_out = d_pm;
    p.ad_retry = h->d_flags.p; p.ad_stage = d_stage; p.ad_crc = d_crc_ok; p.ad_s = 0; p.ad_last = 0;
    // the prefix pass serves stage 0 alone: its buffer is per row of the full batch for groups of g[0].gs lanes; the later stages
    // walk from leaf 0, as the fallback pass does
    PolarAdaptParams p0 = p;
    if ((rc = prefix_params(h, g[0].gs, p0))) return rc;
    unsigned int *ctl = h->d_adapt_ctl.p;
    HIP_TRY(hipMemsetAsync(ctl, 0, kCtlWords * sizeof(unsigned int), st));
    if (p0.prefix_q) HIP_TRY(polar_launch_prefix(p0, false, nullptr, st));
    for (int s = 0; s < n_s; ++s) {
        PolarAdaptParams ps = s ? p : p0;
        ps.L = Ls[s]; ps.work = ctl + s; ps.ad_s = s; ps.ad_last = (s == n_s - 1) ? 1 : 0;
        if (s) { ps.cw_list = h->d_list.p; ps.cw_count = ctl + kCtlCount + (s - 1); }
        HIP_TRY(polar_launch_decode_llr_adapt(ps, g[s].gs, g[s].grid, st));
        // (every decoded codeword rewrote its retry byte, every other one keeps the 0 of the stage that delivered it: the bytes
        // of all B rows are this stage's verdicts)
        if (s < n_s - 1) HIP_TRY(polar_launch_ed_collect(h->d_flags.p, B, nullptr, h->d_list.p, ctl + kCtlCount + s, st));
    }
    return POLAR_OK;
}

}  // namespace

extern "C" {

int polar_decode_scl_llr_adaptive_batch_dev(polar_code_t *h, const void *d_llr, int fmt, long B, const uint8_t *Ls, int n_s,
                                            uint8_t *d_out, double *d_pm, uint8_t *d_stage, uint8_t *d_crc_ok, void *stream) {
    return on_device(h, adaptive_check(h, d_llr, fmt, B, Ls, n_s, d_out), B, [&] {
        return adaptive_launch(h, d_llr, fmt, B, Ls, n_s, d_out, d_pm, d_stage, d_crc_ok, (hipStream_t)stream);
    });
}

// One copy in, the stages, a wait, the copies out.
int polar_decode_scl_llr_adaptive_batch(polar_code_t *h, const void *llr, int fmt, long B, const uint8_t *Ls, int n_s, uint8_t *out,
                                        double *pm, uint8_t *stage, uint8_t *crc_ok) {
    return on_device(h, adaptive_check(h, llr, fmt, B, Ls, n_s, out), B, [&]() -> int {
        int rc;
        const size_t K = (size_t)h->K;
        if ((rc = stage_rows(h, llr, fmt, B))) return rc;
        if ((rc = h->d_out.ensure((size_t)B * K))) return rc;
        if ((rc = h->d_bytes_b.ensure(2 * (size_t)B))) return rc;
        if ((rc = h->d_list_out.ensure((size_t)B))) return rc;
        uint8_t *d_stage = h->d_bytes_b.p, *d_crc = d_stage + B;
        if ((rc = adaptive_launch(h, h->d_in.p, fmt, B, Ls, n_s, h->d_out.p, pm ? h->d_list_out.p : nullptr, stage ? d_stage : nullptr,
                                  crc_ok ? d_crc : nullptr, nullptr))) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        if ((rc = copy_back(out, 0, h->d_out.p, (size_t)B * K)) || (rc = copy_back(pm, 0, h->d_list_out.p, (size_t)B))) return rc;
        if ((rc = copy_back(stage, 0, d_stage, (size_t)B))) return rc;
        return copy_back(crc_ok, 0, d_crc, (size_t)B);
    });
}

// Per enabled point and per chunk of trials, stream-ordered: the trials' LLRs and sent info (synth_kernel), the stages, the
// classification. The counters stay on the device until the end.
int polar_mc_batch_adaptive(polar_code_t *h, int constellation, uint64_t seed, uint64_t t0, long T, long stride, const double *axis,
                            int n_e, const uint8_t *Ls, int n_s, const uint8_t *enabled, uint64_t *stats) {
    Sweep sw;
    int rc = sweep_begin(sw, h, axis && Ls && enabled && stats, "adaptive decoder has", constellation, seed, t0, T, stride, axis, n_e > 0,
                         stats, [&]() -> int {
        if (int r = schedule_check(Ls, n_s)) return r;
        return h->crc ? POLAR_OK : fail(POLAR_E_ARG, "adaptive decoding needs a CRC: this code has none to accept a word on");
    });
    if (rc || T == 0) return rc;
    const int N = h->N, K = h->K, C = POLAR_AD_STAGE0 + n_s;
    const long chunk = sweep_chunk(h, T, (size_t)N * sizeof(double) + 2 * (size_t)K + 2);
    // (every buffer at its largest before the first launch)
    BatchGeometry g[POLAR_AD_MAX_STAGES];
    if ((rc = adaptive_prepare(h, chunk, Ls, n_s, g))) return rc;
    if ((rc = sweep_rows(h, chunk))) return rc;
    if ((rc = h->d_out.ensure((size_t)chunk * K))) return rc;                    // delivered words
    if ((rc = h->d_bytes_b.ensure(2 * (size_t)chunk))) return rc;                // stage, crc_ok
    uint8_t *d_stage = h->d_bytes_b.p, *d_crc = d_stage + chunk;
    const auto cells = sweep_cells(enabled, 1, n_e, C, {chunk});
    return sweep_walk(sw, cells, C, 1, n_e, [&](const SweepCell &cell, long c, const PolarEncodeParams &) -> int {
        if (int r = adaptive_launch(h, h->d_in.p, POLAR_LLR_F64, c, Ls, n_s, h->d_out.p, nullptr, d_stage, d_crc, nullptr)) return r;
        HIP_TRY(polar_launch_adapt_classify(h->d_out.p, d_stage, d_crc, h->d_bytes_a.p, c, K, n_s, h->d_mc_ctr.p + cell.ctr, nullptr));
        return POLAR_OK;
    });
}

}  // extern "C"
