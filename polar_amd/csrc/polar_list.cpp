// polar_list.cpp — list output of decode_scl_llr: every path the list decoder holds at the end of a codeword, with its metric
// and CRC result (include/polar_amd.h polar_decode_scl_llr_list_batch*), and the search for a given word in it.
// One kernel family: the LLR-domain batch kernel with the list-output finish (polar_kernels.hip, POLAR_ED_TU = 4) at the default
// tuning — no exp-domain pass, so no fallback pass; no one-codeword-per-wave form; the handle's mode and tuning are not looked at.
#include "polar_host.h"

namespace {

int list_check(const polar_code *h, const void *llr, int fmt, long B, int L, const uint8_t *cand) {
    return check_args(h && llr && cand, L, B, [&] { return llr_fmt_check(fmt, llr); });
}

// the geometry of a call of B rows and every buffer its launches use at its size — BEFORE the first launch: a DevBuf that grows
// frees what work in flight may still read. p: the parameters but the caller's pointers
int list_prepare(polar_code *h, long B, int L, BatchGeometry &g, PolarListParams &p) {
    if (!batch_geometry(h, B, L, false, g)) return fail(POLAR_E_UNSUPPORTED, "the list kernel's LDS does not fit this device");
    int rc;
    if ((rc = default_scratch(h, &g, 1))) return rc;
    if ((rc = h->d_work.ensure(1))) return rc;
    base_params(h, L, B, p);
    return prefix_params(h, g.gs, p);
}

// (arguments checked, B > 0, the handle's device current)
int list_launch(polar_code *h, const void *d_llr, int fmt, long B, int L, uint8_t *d_cand, double *d_pm, uint8_t *d_crc_ok,
                int32_t *d_n_active, int32_t *d_winner, hipStream_t st) {
    BatchGeometry g; PolarListParams p;
    if (int rc = list_prepare(h, B, L, g, p)) return rc;
    p.llr = (const double *)d_llr; p.llr_fmt = fmt;
    p.list_cand = d_cand; p.list_pm = d_pm; p.list_crc = d_crc_ok; p.list_nact = d_n_active; p.list_win = d_winner;
    HIP_TRY(hipMemsetAsync(p.work, 0, sizeof(unsigned int), st));
    if (p.prefix_q) HIP_TRY(polar_launch_prefix(p, false, nullptr, st));
    HIP_TRY(polar_launch_decode_llr_list(p, g.gs, g.grid, st));
    return POLAR_OK;
}

// One chunk of list output carved out of d_list_out: the metrics (doubles) first, the sent words' metrics where the sweep asks for
// them, the two int32 arrays, then the bytes
struct ListChunk {
    double *pm, *pm_sent; int32_t *n_active, *winner; uint8_t *cand, *crc_ok;
    static size_t per_cw(int L, int K) { return (size_t)L * K + 9 * (size_t)L + 8; }          // bytes of a codeword's list
    static size_t doubles(long chunk, int L, int K, bool sent) { return ((size_t)chunk * per_cw(L, K) + 7) / 8 + 1 + (sent ? (size_t)chunk : 0); }
    ListChunk(double *base, long chunk, int L, int K, bool sent)
        : pm(base), pm_sent(pm + (size_t)chunk * L), n_active(reinterpret_cast<int32_t *>(pm_sent + (sent ? chunk : 0))),
          winner(n_active + chunk), cand(reinterpret_cast<uint8_t *>(winner + chunk)), crc_ok(cand + (size_t)chunk * L * K) {}
};

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
    return on_device(h, list_check(h, d_llr, fmt, B, L, d_cand), B, [&] {
        return list_launch(h, d_llr, fmt, B, L, d_cand, d_pm, d_crc_ok, d_n_active, d_winner, (hipStream_t)stream);
    });
}

// One copy in, then per chunk of codewords: the launches, a wait, the copies out. The chunk bounds the device memory the list
// takes (L K + 9 L + 8 bytes per codeword), not the input, which is resident for the whole call.
int polar_decode_scl_llr_list_batch(polar_code_t *h, const void *llr, int fmt, long B, int L, uint8_t *cand, double *pm,
                                    uint8_t *crc_ok, int32_t *n_active, int32_t *winner) {
    return on_device(h, list_check(h, llr, fmt, B, L, cand), B, [&]() -> int {
        int rc;
        if ((rc = stage_rows(h, llr, fmt, B))) return rc;
        const size_t row = (size_t)h->N * polar_llr_esz(fmt), LK = (size_t)L * h->K;
        const long chunk = chunk_len(h, B, (size_t)256 << 20, ListChunk::per_cw(L, h->K));
        if ((rc = h->d_list_out.ensure(ListChunk::doubles(chunk, L, h->K, false)))) return rc;
        const ListChunk d(h->d_list_out.p, chunk, L, h->K, false);
        for (long b0 = 0; b0 < B; b0 += chunk) {
            const long c = std::min(chunk, B - b0);
            if ((rc = list_launch(h, reinterpret_cast<const char *>(h->d_in.p) + (size_t)b0 * row, fmt, c, L, d.cand, pm ? d.pm : nullptr,
                                  crc_ok ? d.crc_ok : nullptr, n_active ? d.n_active : nullptr, winner ? d.winner : nullptr, nullptr))) return rc;
            HIP_TRY(hipStreamSynchronize(nullptr));
            if ((rc = copy_back(cand, (size_t)b0 * LK, d.cand, (size_t)c * LK)) || (rc = copy_back(pm, (size_t)b0 * L, d.pm, (size_t)c * L)) ||
                (rc = copy_back(crc_ok, (size_t)b0 * L, d.crc_ok, (size_t)c * L)) || (rc = copy_back(n_active, (size_t)b0, d.n_active, (size_t)c)) ||
                (rc = copy_back(winner, (size_t)b0, d.winner, (size_t)c))) return rc;
        }
        return POLAR_OK;
    });
}

int polar_list_find_dev(polar_code_t *h, const uint8_t *d_cand, const int32_t *d_n_active, const uint8_t *d_info, long B, int L,
                        int32_t *d_rank, void *stream) {
    return on_device(h, check_args(h && d_cand && d_n_active && d_info && d_rank, L, B), B, [&]() -> int {
        HIP_TRY(polar_launch_list_find(d_cand, d_n_active, d_info, B, L, h->K, d_rank, (hipStream_t)stream));
        return POLAR_OK;
    });
}

int polar_path_metric_batch_dev(polar_code_t *h, const void *d_llr, int fmt, const uint8_t *d_info, long B, int R, double *d_pm, void *stream) {
    return on_device(h, metric_check(h, d_llr, fmt, d_info, B, R, d_pm), B, [&] {
        return metric_launch(h, d_llr, fmt, d_info, B, R, d_pm, (hipStream_t)stream);
    });
}

int polar_path_metric_batch(polar_code_t *h, const void *llr, int fmt, const uint8_t *info, long B, int R, double *pm) {
    return on_device(h, metric_check(h, llr, fmt, info, B, R, pm), B, [&]() -> int {
        int rc;
        const size_t words = (size_t)B * R;
        if ((rc = stage_rows(h, llr, fmt, B))) return rc;
        if ((rc = h->d_bytes_b.ensure(words * h->K))) return rc;
        if ((rc = h->d_list_out.ensure(words))) return rc;
        HIP_TRY(hipMemcpy(h->d_bytes_b.p, info, words * h->K, hipMemcpyHostToDevice));
        if ((rc = metric_launch(h, h->d_in.p, fmt, h->d_bytes_b.p, B, R, h->d_list_out.p, nullptr))) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        return copy_back(pm, 0, h->d_list_out.p, words);
    });
}

// Per enabled (list size, point) and per chunk of trials, stream-ordered: the trials' LLRs and sent info (synth_kernel), the list
// decode, the sent word's own metric (one word per row), the classification. The counters stay on the device until the end.
int polar_mc_batch_list(polar_code_t *h, int constellation, uint64_t seed, uint64_t t0, long T, long stride, const double *axis, int n_e,
                        const uint8_t *L, int n_L, const uint8_t *enabled, uint64_t *stats) {
    Sweep sw;
    int rc = sweep_begin(sw, h, axis && L && enabled && stats, "list statistics have", constellation, seed, t0, T, stride, axis,
                         n_e > 0 && n_L > 0, stats, [&] { return check_list_sizes(L, n_L); });
    if (rc || T == 0) return rc;
    // (every buffer at its largest before the first launch: the decode's own per list size, the chunks of rows, sent info and output)
    std::vector<long> chunk(n_L);
    size_t out_max = 0;
    for (int li = 0; li < n_L; ++li) {
        chunk[li] = chunk_len(h, T, (size_t)256 << 20, ListChunk::per_cw(L[li], h->K));
        BatchGeometry g; PolarListParams p;
        if ((rc = list_prepare(h, chunk[li], L[li], g, p))) return rc;
        out_max = std::max(out_max, ListChunk::doubles(chunk[li], L[li], h->K, true));
    }
    if ((rc = sweep_rows(h, *std::max_element(chunk.begin(), chunk.end())))) return rc;
    if ((rc = h->d_list_out.ensure(out_max))) return rc;
    const auto cells = sweep_cells(enabled, n_L, n_e, POLAR_LS_N, chunk);
    return sweep_walk(sw, cells, POLAR_LS_N, n_L, n_e, [&](const SweepCell &cell, long c, const PolarEncodeParams &) -> int {
        const int Ls = L[cell.row];
        const ListChunk d(h->d_list_out.p, cell.chunk, Ls, h->K, true);
        if (int r = list_launch(h, h->d_in.p, POLAR_LLR_F64, c, Ls, d.cand, d.pm, d.crc_ok, d.n_active, d.winner, nullptr)) return r;
        if (int r = metric_launch(h, h->d_in.p, POLAR_LLR_F64, h->d_bytes_a.p, c, 1, d.pm_sent, nullptr)) return r;
        HIP_TRY(polar_launch_list_classify(d.cand, d.pm, d.crc_ok, d.n_active, d.winner, h->d_bytes_a.p, d.pm_sent, c, Ls, h->K, nullptr,
                                           h->d_mc_ctr.p + cell.ctr, nullptr));
        return POLAR_OK;
    });
}

}  // extern "C"
