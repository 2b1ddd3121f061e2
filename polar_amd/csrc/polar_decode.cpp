// polar_decode.cpp — decode_scl_llr on the device: the family choice (choose_family), one launcher per family behind
// decode_impl, the device-resident entry points, the probability-domain members of the class surface, encoder / workload generation.
// Reference: PolarCode::decode_scl_llr (PolarCode.cpp:130-148), decode_scl_p1 (:110-128), encode (:60-91).
#include "polar_host.h"
#include "polar_head_plan.h"

namespace {

int effective_mode(const polar_code *h) { return h->knobs.mode_override >= 0 ? h->knobs.mode_override : h->mode; }
// waves of the one-codeword-per-wave list kernel the LDS lets the device hold (0: its state does not fit)
long lat_resident(const polar_code *h, int gs) {
    const size_t lds = polar_decode_lat_lds_bytes(h->N, gs, h->W);
    return lds <= h->lds_per_block ? (long)h->num_cu * std::min<long>(4, (long)(h->lds_per_block / lds)) : 0;
}
// list size 1, small batches: one codeword per wave, whole state in LDS (sc_lat_kernel)
bool use_sc_lat(const polar_code *h, long B) {
    return h->n <= polar_sc_lat_max_log() && polar_sc_lat_lds_bytes(h->N, (int)h->sc_lat_ops.size()) <= h->lds_per_block &&
           h->knobs.lat_max_b >= 0 && B <= (h->knobs.lat_max_b ? h->knobs.lat_max_b : 2048);
}

// one decode_impl call as its launchers see it: the arguments, the batch geometry (scratch in place), the call's decode parameters
struct Call {
    polar_code *h;
    const void *d_llr; int llr_fmt; long B; const unsigned int *n_dev; int L; uint8_t *d_out; double *d_pm;
    hipStream_t st; void *ev_start, *ev_stop; int phase; Deferred *deferred;
    BatchGeometry g; PolarDecodeParams p;
};

// the tuned batch geometry and its scratch: when the per-wave state scratch — big * 512 B per resident wave, 1 MiB at N = 2048 —
// has to grow it is capped (scratch_budget) by running fewer persistent waves
int batch_setup(polar_code *h, long B, int L, BatchGeometry &g) {
    if (!batch_geometry(h, B, L, true, g)) return fail(POLAR_E_ARG, "lds_log %d does not fit the LDS", g.lds_log);
    if ((size_t)g.grid * g.big * 64 + 64 > h->d_llr_scr.cap) {
        const size_t per_wave = g.big * 64 * sizeof(double) + 1;
        const long cap = (long)(scratch_budget(h) / per_wave);
        if (g.grid > cap) g.grid = (int)std::max<long>(g.wpb, (cap / g.wpb) * g.wpb);
    }
    return ensure_batch_scratch(h, g);
}

// The fallback pass: the LLR-domain batch kernel, no prefix kernel, at most max_grid waves, over a device-side work list (normally
// empty; no host synchronisation). `work`: its hand-out counter, zeroed by the caller; nullptr: the handle's own, zeroed here.
int fallback_pass(const PolarDecodeParams &p, const BatchGeometry &g, const uint32_t *list, const unsigned int *count, unsigned int *work, int max_grid, hipStream_t st) {
    PolarDecodeParams pf = p;
    pf.prefix_q = 0; pf.prefix_len = 0; pf.pre = nullptr;
    if (work) pf.work = work;
    else HIP_TRY(hipMemsetAsync(pf.work, 0, sizeof(unsigned int), st));
    pf.cw_list = list; pf.cw_count = count; pf.n_dev = nullptr;
    HIP_TRY(polar_launch_decode_llr(pf, g.gs, g.lds_log, g.pipe, std::min(g.grid, max_grid), false, st));
    return POLAR_OK;
}

// ---- list size 1: pruned successive cancellation, eight lanes per codeword (polar_kernels_sc.hip), or for small batches one codeword
// per wave, whole state in LDS (sc_lat_kernel: a lone wave of the eight-codeword kernel pays a memory round trip per dependent access
// of its HBM-resident layers — B = 1: 0.85 ms against 0.33 ms on a host core). Flagged codewords (degenerate inputs, |x| < 40
// decisions too close to call) go through the general kernel in the fallback pass.
int decode_sc8(Call &c, bool lat) {
    polar_code *h = c.h; const BatchGeometry &g = c.g;
    const long B = c.B;
    int rc;
    // (measured and dropped: as many waves as make the rounds of eight-codeword groups whole — 4 096 instead of 5 120 for
    // 65 536 codewords — is 2.5 % SLOWER: the kernel wants the latency hiding of 20 waves per CU more than a full last round)
    const int sgrid = (int)std::min<long>((B + 7) / 8, (long)h->num_cu * polar_sc8_waves_per_cu(h->N));
    // (the in-place reads are 16-byte vector loads: a caller's pointer that is not 16-byte aligned takes the front pass; the knob:
    // A/B measurements and the parity tests of both paths)
    const bool in_place = lat || (h->sc_fold && !h->knobs.sc_no_fold && ((uintptr_t)c.d_llr & 15u) == 0);
    if (!in_place && (rc = h->d_ech.ensure((size_t)B * h->N))) return rc;
    if ((rc = h->d_list.ensure((size_t)B))) return rc;
    // control words and flag words in ONE buffer, zeroed by ONE memset: [0] work counter of the decode kernel, [1] length of
    // the fallback work list, [2] work counter of the fallback pass, [4 ...] one flag bit per codeword (round 3: four
    // memsets and two kernels — bits -> bytes -> list — around the decode kernel; a step at batch 65536 is 3.3 ms)
    const size_t nfw = (size_t)(B + 31) / 32 + 1;
    if ((rc = h->d_flag_words.ensure(4 + nfw))) return rc;
    unsigned int *ctrl = h->d_flag_words.p, *fwords = h->d_flag_words.p + 4;
    // (the alpha scratch is shared with the general kernel's, which the fallback pass uses)
    if ((rc = h->d_llr_scr.ensure(std::max((size_t)sgrid * polar_sc8_scratch_doubles_per_wave(h->N) + 64, (size_t)g.grid * g.big * 64 + 64)))) return rc;
    c.p.llr_scr = h->d_llr_scr.p;
    if (c.phase != 2) {
        HIP_TRY(hipMemsetAsync(ctrl, 0, (4 + nfw) * sizeof(unsigned int), c.st));
        if (!in_place) HIP_TRY(polar_launch_sc8_front(c.d_llr, c.llr_fmt, h->d_ech.p, fwords, h->d_tabs.p, h->n, B, c.n_dev, c.st));
        PolarScParams sp;
        sp.n = h->n; sp.N = h->N; sp.K = h->K; sp.B = B;
        sp.llr = in_place ? c.d_llr : nullptr; sp.llr_fmt = c.llr_fmt;
        sp.ech_t = in_place ? nullptr : h->d_ech.p; sp.out = c.d_out;
        sp.ops = lat ? h->d_sc_lat_ops.p : h->d_sc_ops.p; sp.n_ops = (int)(lat ? h->sc_lat_ops.size() : h->sc_ops.size());
        sp.order = h->d_order.p; sp.tabs = h->d_tabs.p; sp.a_scr = h->d_llr_scr.p;
        sp.flag_words = fwords; sp.work = ctrl; sp.n_dev = c.n_dev;
        sp.flag_bytes = lat ? h->lat_flag_bytes : nullptr;
        if (c.ev_start) HIP_TRY(hipEventRecord((hipEvent_t)c.ev_start, c.st));
        HIP_TRY(lat ? polar_launch_sc_lat(sp, lat_grid(h, std::min<long>(B, (long)h->num_cu * 4)), c.st) : polar_launch_sc8_decode(sp, sgrid, c.st));
        if (c.ev_stop) HIP_TRY(hipEventRecord((hipEvent_t)c.ev_stop, c.st));
        if (c.phase == 1 && lat && c.deferred) { *c.deferred = Deferred::FlagWords; return POLAR_OK; }
    }
    HIP_TRY(polar_launch_sc_collect(fwords, B, c.n_dev, h->d_list.p, ctrl + 1, c.st));
    h->note_fallback(ctrl + 1, h->d_list.p, c.st, B);
    return fallback_pass(c.p, g, h->d_list.p, ctrl + 1, ctrl + 2, 16 * g.wpb, c.st);
}

// ---- small batches of the small lists: ONE codeword per wave, its elements spread over the 64 / gs lanes of each path, the state in
// LDS (scl_decode_llr_kernel<.., LAT = 1>; exp-domain arithmetic for groups of 4 and 8 lanes, LLR-domain for groups of 2). The
// kernel converts the channel itself (no conversion pass, no prefix kernel).
// (groups of 2 lanes: the batch path is the LLR-domain kernel, but ONE codeword per wave is faster with the exp-domain nodes — 2.2
// against 2.9 ms —, unless mode 1 forces the LLR-domain arithmetic, which flags nothing: no fallback pass, no batch geometry. A
// requested path metric takes the LLR-domain form as well: the exp-domain leaf terms are -log(E) where the batch kernel of these
// groups adds |llr|, one ulp apart on a third of the rows, and a row's metric must not depend on how many rows came with it)
int decode_list_lat(const Call &c) {
    polar_code *h = c.h;
    const int gs = pow2ceil(c.L);
    const bool ed = effective_mode(h) != 1 && !(gs == 2 && c.d_pm);
    const long resident = lat_resident(h, gs);
    int rc;
    if (ed) {
        // (sized for the largest batch this path ever takes — a few hundred entries — so that the first call reserves it)
        const size_t cap = (size_t)std::max<long>(c.B, 2 * resident);
        if ((rc = h->d_flags.ensure(cap))) return rc;
        if ((rc = h->d_list.ensure(cap))) return rc;
        if ((rc = h->d_count.ensure(1))) return rc;
    }
    const PolarDecodeParams &p = c.p;
    if (c.phase != 2) {
        PolarDecodeParams pl = p;
        if (ed) pl.flags = h->d_flags.p;
        HIP_TRY(hipMemsetAsync(p.work, 0, sizeof(unsigned int), c.st));
        if (c.ev_start) HIP_TRY(hipEventRecord((hipEvent_t)c.ev_start, c.st));
        HIP_TRY(polar_launch_decode_lat(pl, gs, ed, lat_grid(h, std::min<long>(c.B, resident)), c.st));
        if (c.ev_stop) HIP_TRY(hipEventRecord((hipEvent_t)c.ev_stop, c.st));
        if (ed && c.phase == 1 && c.deferred) { *c.deferred = Deferred::FlagBytes; return POLAR_OK; }
    }
    if (!ed) return POLAR_OK;
    HIP_TRY(hipMemsetAsync(h->d_count.p, 0, sizeof(unsigned int), c.st));
    HIP_TRY(polar_launch_ed_collect(h->d_flags.p, c.B, c.n_dev, h->d_list.p, h->d_count.p, c.st));
    h->note_fallback(h->d_count.p, h->d_list.p, c.st, c.B);
    return fallback_pass(p, c.g, h->d_list.p, h->d_count.p, nullptr, 64 * c.g.wpb, c.st);
}

// ---- the batch kernel, LLR-domain arithmetic: lists of 1 (with a path metric) and 2, and every list in mode 1
int decode_batch_llr(Call &c) {
    polar_code *h = c.h; const BatchGeometry &g = c.g;
    PolarDecodeParams &p = c.p;
    if (int rc = prefix_params(h, g.gs, p)) return rc;
    HIP_TRY(hipMemsetAsync(p.work, 0, sizeof(unsigned int), c.st));
    if (p.prefix_q) HIP_TRY(polar_launch_prefix(p, false, nullptr, c.st));
    if (c.ev_start) HIP_TRY(hipEventRecord((hipEvent_t)c.ev_start, c.st));
    HIP_TRY(polar_launch_decode_llr(p, g.gs, g.lds_log, g.pipe, g.grid, false, c.st));
    if (c.ev_stop) HIP_TRY(hipEventRecord((hipEvent_t)c.ev_stop, c.st));
    return POLAR_OK;
}

// ---- the batch kernel, exp-domain arithmetic (one division per f-node instead of four transcendentals) for the list sizes
// where the f-node dominates; codewords it flags (decisions within 1e-10 of the |x| < 40 test, degenerate inputs) are decoded
// again by the LLR-domain kernel in the fallback pass.
int decode_batch_ed(Call &c) {
    polar_code *h = c.h; const BatchGeometry &g = c.g;
    PolarDecodeParams &p = c.p;
    const long B = c.B;
    int rc;
    if ((rc = prefix_params(h, g.gs, p))) return rc;
    HIP_TRY(hipMemsetAsync(p.work, 0, 2 * sizeof(unsigned int), c.st));          // (the second word: phase A of the two-phase form)
    if ((rc = h->d_ech.ensure((size_t)B * h->N))) return rc;
    if ((rc = h->d_flags.ensure((size_t)B))) return rc;
    if ((rc = h->d_list.ensure((size_t)B))) return rc;
    if ((rc = h->d_count.ensure(1))) return rc;
    HIP_TRY(hipMemsetAsync(h->d_count.p, 0, sizeof(unsigned int), c.st));
    // (round 4: where the prefix kernel's first pass is staged through LDS it converts the raw rows itself — no conversion pass)
    const bool fuse_front = p.prefix_q > 0 && polar_prefix_is_staged(h->N) && !h->knobs.no_fuse_front;
    if (!fuse_front) HIP_TRY(polar_launch_ed_front(c.d_llr, c.llr_fmt, h->d_ech.p, h->d_flags.p, h->d_tabs.p, h->N, B, c.n_dev, c.st));
    PolarDecodeParams pe = p;
    pe.llr = h->d_ech.p; pe.llr_fmt = POLAR_LLR_F64; pe.flags = h->d_flags.p;
    if (g.gs == 32 && !g.pipe && h->N >= 1024 && p.prefix_q > 0 && !h->knobs.no_tables) {
        // table mode: layers 1 and 2 as per-codeword value tables (polar_kernels.hip)
        if ((rc = h->d_tab_scr.ensure((size_t)g.grid * g.G * 3 * h->N + 64))) return rc;
        if ((rc = h->d_var_scr.ensure((size_t)g.grid * (h->N / 32) * 64 + 64))) return rc;
        pe.tab_scr = h->d_tab_scr.p; pe.var_scr = h->d_var_scr.p;
    }
    if (pe.prefix_q && fuse_front) {
        PolarDecodeParams pp = pe;
        pp.llr = (const double *)c.d_llr; pp.llr_fmt = c.llr_fmt;
        HIP_TRY(polar_launch_prefix(pp, true, h->d_ech.p, c.st));
    } else if (pe.prefix_q) HIP_TRY(polar_launch_prefix(pe, true, nullptr, c.st));
    // Two phases (polar_head_plan.h): up to the third unfrozen leaf a codeword has at most 4 paths — those leaves go through the
    // 4-lane instantiation, 16 codewords a wave, which leaves a record per codeword; the list of 32 starts there. Same stream, same
    // scratch (the phases are sequential), a work counter each. Table mode starts with the build at N/2 when the hand-over lies in
    // the second quarter (the walk has no table of the first build then), so the hand-over stays below N/2.
    HeadPlan hp;
    if (g.gs == 32 && p.prefix_q > 0) hp = head_plan(h->frozen.data(), h->n, p.prefix_q, p.prefix_len, h->N / 2);
    const long head_min_b = h->knobs.head_min_b ? h->knobs.head_min_b : (long)h->num_cu * 16 * 16;
    const bool two_phase = head_use(hp, g.lds_log == 3 && !g.pipe, B, head_min_b, h->knobs.no_head);
    h->last_head_phi = two_phase ? hp.phi_h : 0;
    h->last_head_b = two_phase && !c.n_dev ? B : 0;
    PolarHeadParams ph;
    if (two_phase) {
        if ((rc = h->d_head_rec.ensure((size_t)B * hp.record_words()))) return rc;
        static_cast<PolarDecodeParams &>(ph) = pe;
        ph.head_rec = h->d_head_rec.p; ph.head_phi = hp.phi_h; ph.head_t = hp.t; ph.head_rows = hp.rows();
        ph.head_llr_mask = hp.llr_mask; ph.head_c_mask = hp.c_mask;
    }
    if (c.ev_start) HIP_TRY(hipEventRecord((hipEvent_t)c.ev_start, c.st));
    if (two_phase) {
        PolarHeadParams pa = ph;
        pa.L = HeadPlan::kPaths; pa.work = p.work + 1; pa.tab_scr = nullptr; pa.var_scr = nullptr; pa.out = nullptr; pa.pm_out = nullptr;
        const long waves_a = (B + 15) / 16;
        const int grid_a = (int)std::min<long>(g.grid, ((waves_a + g.wpb - 1) / g.wpb) * g.wpb);
        HIP_TRY(polar_launch_decode_head_export(pa, grid_a, c.st));
        HIP_TRY(polar_launch_decode_head_import(ph, g.grid, c.st));
    } else
    HIP_TRY(polar_launch_decode_llr(pe, g.gs, g.lds_log, g.pipe, g.grid, true, c.st));
    if (c.ev_stop) HIP_TRY(hipEventRecord((hipEvent_t)c.ev_stop, c.st));
    HIP_TRY(polar_launch_ed_collect(h->d_flags.p, B, c.n_dev, h->d_list.p, h->d_count.p, c.st));
    // (normally empty: a few blocks; a code with weak unfrozen leaves may send most of its codewords here)
    h->note_fallback(h->d_count.p, h->d_list.p, c.st, B);
    return fallback_pass(p, g, h->d_list.p, h->d_count.p, nullptr, h->weak_leaves ? g.grid : 64 * g.wpb, c.st);
}

}  // namespace

Family polar_host::choose_family(const polar_code *h, long B, int L, bool want_pm) {
    const int mode = effective_mode(h), gs = pow2ceil(L);
    // (a requested path metric needs the general kernel: the list-size-1 kernels have none)
    if (L == 1 && mode != 1 && !want_pm) return use_sc_lat(h, B) ? Family::ScLat : Family::Sc8;
    // (the exp-domain kernels exist for groups of 4 lanes and more: smaller lists take the LLR-domain kernel in every mode)
    // (round 3: automatic mode takes the exp-domain kernel from lists of 3 on — it was 5: with the block-placement hints the
    // 4-lane groups run 16 % faster on it, config 3: 4.4 -> 5.1 M cw/s)
    const bool ed = gs >= 4 && mode != 1;
    // (measured, N = 2048, round 6 — profiles/r06/latency_table_248.json: L = 4 B = 1 ... 256 1.80 ... 1.94 ms against 3.80 ... 4.36 ms
    // for the batch kernel, L = 2 1.73 ... 2.09 against 5.9 ... 7.0 ms, L = 8 2.02 ... 2.17 against 3.83 ... 4.40. The LDS lets the
    // device hold one wave per CU for lists of 4 and 8 at N = 2048, three for lists of 2; TWO rounds of that are still faster than
    // the batch kernel — B = 512: 3.80 against 4.46 ms at L = 4, 4.25 against 4.59 at L = 8; B = 1024: 4.10 against 7.24 at L = 2 —,
    // three are not: that is the default threshold)
    const long resident = lat_resident(h, gs);
    if ((gs == 2 || (ed && (gs == 4 || gs == 8))) && h->knobs.lat_max_b >= 0 && resident > 0 &&
        B <= (h->knobs.lat_max_b ? h->knobs.lat_max_b : 2 * resident)) return Family::ListLat;
    return ed ? Family::BatchEd : Family::BatchLlr;
}

// all-frozen prefix [0, P): handled cooperatively by the kernel when one codeword owns 32 lanes
int polar_host::prefix_params(polar_code *h, int gs, PolarDecodeParams &p) {
    int P = 0;
    while (P < h->N && h->frozen[P]) ++P;
    int Q = 0;
    if (gs >= 4 && h->prefix_on) {
        if (P >= 256) Q = 256;
        else { Q = 64; while (Q <= P) Q <<= 1; if (P < 33) Q = 0; }
        if (Q > h->N / 2) Q = 0;
    }
    p.prefix_q = Q; p.prefix_len = Q ? std::min(P, Q) : 0;
    if (!Q) return POLAR_OK;
    if (int rc = h->d_pre.ensure((size_t)p.B * (size_t)(h->N - Q + 1))) return rc;
    p.pre = h->d_pre.p;
    return POLAR_OK;
}

bool polar_host::batch_geometry(const polar_code *h, long B, int L, bool tuned, BatchGeometry &g) {
    g.gs = pow2ceil(L); g.G = 64 / g.gs;
    const long groups = (B + g.G - 1) / g.G;
    // two tuned variants: "pipe" (8 waves/CU, S<=16 in LDS, register double-buffering) and the
    // default high-occupancy one (4-wave blocks, S<=8 in LDS, 16 waves/CU)
    g.wpc = tuned && h->waves_per_cu ? h->waves_per_cu : 16;
    int lds_log = tuned ? h->lds_log : 3;
    // Small batches of the large lists (no one-codeword-per-wave form: their state does not fit the LDS), round 6: when every group
    // of the call is resident at ONE wave per SIMD anyway, fewer and fatter waves — layers up to 32 in LDS, the register-double-
    // buffered form — answer sooner: a lone wave pays a memory round trip per dependent access of an HBM-resident layer
    // (profiles/r06/small_batch_geometry.txt: L = 32 B = 256 5.10 -> 4.48 ms, L = 16 B = 1024 5.07 -> 4.64; nothing at 4096).
    if (tuned && !h->waves_per_cu && !h->lds_log && g.gs >= 16 && groups <= (long)h->num_cu * 4 &&
        polar_decode_lds_bytes(5, 1) <= h->lds_per_block) { g.wpc = 4; lds_log = 5; }
    g.pipe = (g.wpc > 8) ? 0 : 1;
    g.lds_log = lds_log ? lds_log : (g.pipe ? 4 : 3);
    g.wpb = polar_decode_waves_per_block(g.pipe);
    const int max_blocks_by_lds = (int)(h->lds_per_block / polar_decode_lds_bytes(g.lds_log, g.pipe));
    if (max_blocks_by_lds < 1) return false;
    if (g.wpc > max_blocks_by_lds * g.wpb) g.wpc = max_blocks_by_lds * g.wpb;
    g.grid = (int)std::min(groups, (long)h->num_cu * g.wpc);
    g.grid = ((g.grid + g.wpb - 1) / g.wpb) * g.wpb;          // whole blocks
    g.big = polar_decode_big(h->N, g.lds_log);
    g.cwords = polar_decode_cwords(h->N);
    return true;
}

int polar_host::ensure_batch_scratch(polar_code *h, const BatchGeometry &g) {
    int rc;
    if ((rc = h->d_llr_scr.ensure((size_t)g.grid * g.big * 64 + 64))) return rc;
    if ((rc = h->d_c_scr.ensure((size_t)g.grid * 2 * g.cwords * 64 + 64))) return rc;
    return h->d_hist_scr.ensure((size_t)g.grid * 3 * h->W * 64 + 64);
}

// batch_setup's counterpart at the default tuning (the geometries differ in their grid alone): no budget, the grid halved in whole blocks
int polar_host::default_scratch(polar_code *h, BatchGeometry *g, int n) {
    BatchGeometry gm = *std::max_element(g, g + n, [](const BatchGeometry &a, const BatchGeometry &b) { return a.grid < b.grid; });
    int rc;
    while ((rc = ensure_batch_scratch(h, gm)) == POLAR_E_NOMEM && gm.grid > gm.wpb) {
        (void)hipGetLastError();
        gm.grid = std::max(gm.wpb, (gm.grid / 2 / gm.wpb) * gm.wpb);
    }
    for (int s = 0; s < n && !rc; ++s) g[s].grid = std::min(g[s].grid, gm.grid);
    return rc;
}

void polar_host::base_params(const polar_code *h, int L, long B, PolarDecodeParams &p) {
    p.n = h->n; p.N = h->N; p.K = h->K; p.crc = h->crc; p.L = L; p.W = h->W; p.B = B;
    p.prefix_q = 0; p.prefix_len = 0; p.pre = nullptr;
    p.llr = nullptr; p.llr_fmt = POLAR_LLR_F64; p.p0 = nullptr; p.out = nullptr; p.pm_out = nullptr;
    p.frozen = h->d_frozen.p; p.info_rank = h->d_info_rank.p; p.crc_mask = h->d_crc_mask.p; p.tabs = h->d_tabs.p;
    p.ctl = h->knobs.no_r1 ? h->d_ctl.p : h->d_ctl_r1.p; p.work = h->d_work.p; p.llr_scr = h->d_llr_scr.p; p.c_scr = h->d_c_scr.p; p.hist_scr = h->d_hist_scr.p;
    p.flags = nullptr; p.cw_list = nullptr; p.cw_count = nullptr; p.n_dev = nullptr; p.tab_scr = nullptr; p.var_scr = nullptr;
}

void polar_host::fill_enc(const polar_code *h, PolarEncodeParams &p) {
    memset(&p, 0, sizeof p);
    p.n = h->n; p.N = h->N; p.K = h->K; p.crc = h->crc;
    p.order = h->d_order.p; p.crcm = h->d_crcm.p;
    p.stride = 1;
    p.info_block_div = 100;
}

int polar_host::decode_impl(polar_code *h, const void *d_llr, int llr_fmt, long B, const unsigned int *n_dev, int L, uint8_t *d_out,
                            double *d_pm, void *stream, void *ev_start, void *ev_stop, int phase, Deferred *deferred) {
    if (deferred) *deferred = Deferred::None;
    int rc = check_args(h && d_llr && d_out, L, B);
    if (rc || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    if ((rc = h->d_work.ensure(2))) return rc;
    h->last_head_phi = 0; h->last_head_b = 0;
    if (phase != 2) h->last_lane_waves = 0;
    if (phase != 2) h->last_lat_waves = 0;          // (phase 2 is the fallback pass of the same call: the launch was phase 1's)
    if (phase != 2) h->note_fallback(nullptr, nullptr, nullptr, 0);
    const Family fam = choose_family(h, B, L, d_pm != nullptr);
    Call c{h, d_llr, llr_fmt, B, n_dev, L, d_out, d_pm, (hipStream_t)stream, ev_start, ev_stop, phase, deferred, {}, {}};
    // (every family but one ends in a fallback pass of the batch kernel: the small lists in LLR-domain arithmetic flag nothing)
    if (!(fam == Family::ListLat && effective_mode(h) == 1) && (rc = batch_setup(h, B, L, c.g))) return rc;
    base_params(h, L, B, c.p);
    c.p.llr = (const double *)d_llr; c.p.llr_fmt = llr_fmt; c.p.out = d_out; c.p.pm_out = d_pm; c.p.n_dev = n_dev;
    switch (fam) {
        case Family::Sc8: case Family::ScLat: return decode_sc8(c, fam == Family::ScLat);
        case Family::ListLat: return decode_list_lat(c);
        case Family::BatchLlr: return decode_batch_llr(c);
        case Family::BatchEd: break;
    }
    return decode_batch_ed(c);
}

extern "C" {

int polar_decode_scl_llr_batch_dev(polar_code_t *h, const double *d_llr, long B, int L, uint8_t *d_out,
                                   double *d_pm, void *stream) {
    return polar_decode_scl_llr_batch_dev_fmt(h, d_llr, POLAR_LLR_F64, B, L, d_out, d_pm, stream);
}

int polar_decode_scl_llr_batch_dev_ev(polar_code_t *h, const double *d_llr, long B, int L, uint8_t *d_out,
                                      double *d_pm, void *stream, void *ev_start, void *ev_stop) {
    return decode_impl(h, d_llr, 0, B, nullptr, L, d_out, d_pm, stream, ev_start, ev_stop);
}

// single-precision LLRs at the boundary: every float is widened (exactly) in the load stage of the first kernel that
// touches the channel values (ed_front_kernel / prefix_kernel / the layer-1 visits) — no staging copy
int polar_decode_scl_llr_batch_dev_f32(polar_code_t *h, const float *d_llr, long B, int L, uint8_t *d_out,
                                       double *d_pm, void *stream) {
    return polar_decode_scl_llr_batch_dev_fmt(h, d_llr, POLAR_LLR_F32, B, L, d_out, d_pm, stream);
}
// any element format (POLAR_LLR_*): 16-bit rows are bit patterns, widened exactly by integer operations in the same loads
int polar_decode_scl_llr_batch_dev_fmt(polar_code_t *h, const void *d_llr, int fmt, long B, int L, uint8_t *d_out,
                                       double *d_pm, void *stream) {
    int rc = llr_fmt_check(fmt, d_llr);
    if (rc) return rc;
    return decode_impl(h, d_llr, fmt, B, nullptr, L, d_out, d_pm, stream, nullptr, nullptr);
}

// PolarCode::decode_scl_p1 (PolarCode.cpp:110-128): probability-domain SCL
int polar_decode_scl_p1_batch(polar_code_t *h, const double *p1, const double *p0, long B, int L, uint8_t *out) {
    int rc = check_args(h && p1 && p0 && out, L, B);
    if (rc || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    const int N = h->N;
    const int gs = pow2ceil(L), G = 64 / gs;
    long groups = (B + G - 1) / G;
    // (one wave per block, the whole state in a per-wave scratch of 2 N rows: 16 waves per CU hide its latency — round 4 launched 4 —
    // as long as the scratch of all of them stays below 24 GiB)
    if ((rc = h->d_in.ensure((size_t)B * N * 2))) return rc;
    if ((rc = h->d_out.ensure((size_t)B * h->K))) return rc;
    int grid = 1;
    h->last_lat_waves = 0; h->last_lane_waves = 0;
    rc = grid_that_fits(h, lane_grid(h, std::min<long>(groups, (long)h->num_cu * 16)), (size_t)N * 64 * 2 * sizeof(double), [&](int g) {
        int r = h->d_llr_scr.ensure((size_t)g * N * 64 * 2 + 64);
        if (!r) r = h->d_c_scr.ensure((size_t)g * 2 * polar_decode_cwords(N) * 64 + 64);
        if (!r) r = h->d_hist_scr.ensure((size_t)g * h->W * 64 + 64);
        return r;
    }, &grid);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(h->d_in.p, p1, (size_t)B * N * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_in.p + (size_t)B * N, p0, (size_t)B * N * sizeof(double), hipMemcpyHostToDevice));
    PolarDecodeParams p;
    base_params(h, L, B, p);
    p.ctl = nullptr; p.work = nullptr;          // (the probability-domain kernel has no leaf schedule and no dynamic hand-out)
    p.llr = h->d_in.p; p.p0 = h->d_in.p + (size_t)B * N; p.out = h->d_out.p;
    HIP_TRY(polar_launch_decode_p1(p, gs, grid, nullptr));
    h->last_lane_waves = grid;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, h->d_out.p, (size_t)B * h->K, hipMemcpyDeviceToHost));
    return POLAR_OK;
}
int polar_decode_scl_p1(polar_code_t *h, const double *p1, const double *p0, int L, uint8_t *out) {
    return polar_decode_scl_p1_batch(h, p1, p0, 1, L, out);
}

// PolarM decode_sc_p1 (PolarCode.m:290-295): out are doubles like MATLAB's (0.5 when a leaf is exactly 0.5, NaN when a leaf is NaN)
int polar_decode_sc_p1_batch(polar_code_t *h, const double *p1, long B, double *out) {
    int rc = check_args(h && p1 && out, kNoList, B);
    if (rc || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    const int N = h->N;
    h->last_lat_waves = 0; h->last_lane_waves = 0;
    if ((rc = h->d_in.ensure((size_t)B * N + (size_t)B * h->K))) return rc;
    PolarScP1Params p;
    p.n = h->n; p.N = N; p.K = h->K; p.B = B;
    p.p1 = h->d_in.p; p.out = h->d_in.p + (size_t)B * N;
    p.frozen = h->d_frozen.p; p.order = h->d_order.p; p.scr = nullptr;
    HIP_TRY(hipMemcpy(h->d_in.p, p1, (size_t)B * N * sizeof(double), hipMemcpyHostToDevice));
    // Small batches (PolarM calls this once per codeword, main_MC_CC_Comparison.m:96): one codeword per WAVE, state in LDS; from
    // about one codeword per lane of the waves the device holds the lane-per-codeword kernel wins (its 64 codewords per wave
    // share every instruction). Same doubles either way.
    const long lat_waves = polar_sc_p1_lat_lds_bytes(N) <= h->lds_per_block ? (long)h->num_cu * std::max<long>(1, (long)(h->lds_per_block / polar_sc_p1_lat_lds_bytes(N))) : 0;
    const long lat_max = h->knobs.lat_max_b < 0 ? 0 : (h->knobs.lat_max_b ? h->knobs.lat_max_b : lat_waves * 4);
    if (lat_waves > 0 && B <= lat_max) {
        HIP_TRY(polar_launch_sc_p1_lat(p, lat_grid(h, std::min<long>(B, lat_waves)), nullptr));
    } else {
        int grid = 1;
        rc = grid_that_fits(h, lane_grid(h, std::min<long>((B + 63) / 64, (long)h->num_cu * 16)), (size_t)N * 64 * 4 * sizeof(double),
                            [&](int g) { return h->d_llr_scr.ensure((size_t)g * 4 * N * 64 + 64); }, &grid);
        if (rc) return rc;
        p.scr = h->d_llr_scr.p;
        HIP_TRY(polar_launch_sc_p1(p, grid, nullptr));
        h->last_lane_waves = grid;
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, p.out, (size_t)B * h->K * sizeof(double), hipMemcpyDeviceToHost));
    return POLAR_OK;
}
int polar_decode_sc_p1(polar_code_t *h, const double *p1, double *out) { return polar_decode_sc_p1_batch(h, p1, 1, out); }

int polar_encode_batch_dev(polar_code_t *h, const uint8_t *d_info, long B, uint8_t *d_coded, void *stream) {
    int rc = check_args(h && d_info && d_coded, kNoList, B);
    if (rc || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    PolarEncodeParams p;
    fill_enc(h, p);
    p.B = B; p.info = d_info; p.coded = d_coded;
    HIP_TRY(polar_launch_encode(p, (hipStream_t)stream));
    return POLAR_OK;
}

int polar_encode_batch(polar_code_t *h, const uint8_t *info, long B, uint8_t *coded) {
    int rc = check_args(h && info && coded, kNoList, B);
    if (rc || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    if ((rc = h->d_bytes_a.ensure((size_t)B * h->K))) return rc;
    if ((rc = h->d_bytes_b.ensure((size_t)B * h->N))) return rc;
    HIP_TRY(hipMemcpy(h->d_bytes_a.p, info, (size_t)B * h->K, hipMemcpyHostToDevice));
    if ((rc = polar_encode_batch_dev(h, h->d_bytes_a.p, B, h->d_bytes_b.p, nullptr))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(coded, h->d_bytes_b.p, (size_t)B * h->N, hipMemcpyDeviceToHost));
    return POLAR_OK;
}
int polar_encode(polar_code_t *h, const uint8_t *info, uint8_t *coded) { return polar_encode_batch(h, info, 1, coded); }

int polar_synth_llr_dev(polar_code_t *h, uint64_t seed, uint64_t trial0, long B, double s,
                        double *d_llr, uint8_t *d_info, void *stream) {
    int rc = check_args(h && d_llr, kNoList, B);
    if (rc || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    PolarEncodeParams p;
    fill_enc(h, p);
    p.B = B; p.seed = seed; p.trial0 = trial0; p.s = s; p.llr = d_llr; p.info_out = d_info;
    HIP_TRY(polar_launch_synth(p, (hipStream_t)stream));
    return POLAR_OK;
}

// Pre-size every device scratch buffer decodes of up to B codewords at list sizes 1 .. L need, by running one decode per
// kernel family on generated inputs (list size 1: the pruned SC kernel and its flag words; 2: the LLR-domain kernel's 2-lane
// groups; every power-of-two lane group up to pow2ceil(L), with and without the path-metric output): afterwards
// polar_decode_scl_llr_batch_dev* calls within (B, L) allocate nothing (no hipFree / hipMalloc, i.e. no implicit device
// synchronisation, inside the nominally asynchronous calls; polar_debug_get "allocs" counts them).
int polar_reserve(polar_code_t *h, long B, int L) {
    if (!h) return fail(POLAR_E_ARG, "NULL handle");
    int rc = check_args(true, L, B);
    if (rc || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    DevBuf<double> llr, pm;
    DevBuf<uint8_t> out;
    if ((rc = llr.ensure((size_t)B * h->N + 1)) || (rc = out.ensure((size_t)B * h->K)) || (rc = pm.ensure((size_t)B))) { llr.release(); out.release(); pm.release(); return rc; }
    rc = polar_synth_llr_dev(h, 1, 0, B, polar_snr_sqrt_linear(h, 2.0), llr.p, nullptr, nullptr);
    const int top = std::min(pow2ceil(L), POLAR_MAX_LIST);
    // every kernel family a call within (B, L) can reach: per list size the batch kernel at B and the one-codeword-per-wave
    // kernel at one codeword (its flag / work-list buffers are its own: polar_reserve(B, 2) above the latency threshold used
    // to leave them to the first small call), list size 1 also with a requested metric (the general kernel) and from rows
    // that are NOT 16-byte aligned (the converted copy the in-place reads cannot serve)
    for (int l = 1; l <= top && !rc; l <<= 1) {
        rc = polar_decode_scl_llr_batch_dev(h, llr.p, B, l, out.p, nullptr, nullptr);
        if (!rc && l <= 8) rc = polar_decode_scl_llr_batch_dev(h, llr.p, 1, l, out.p, nullptr, nullptr);
        if (!rc && l == 1) rc = polar_decode_scl_llr_batch_dev(h, llr.p, B, l, out.p, pm.p, nullptr);
        if (!rc && l == 1) rc = polar_decode_scl_llr_batch_dev(h, llr.p + 1, B, l, out.p, nullptr, nullptr);
    }
    // the hand-over records of the two-phase list of 32, whatever the knobs and the batch threshold let the decode above do: a
    // later call within (B, L) that does take the head (another "no_head" / "head_min_b") must not allocate either
    if (!rc && top >= 32) {
        PolarDecodeParams pp;
        base_params(h, 32, B, pp);
        if (!(rc = prefix_params(h, 32, pp)) && pp.prefix_q > 0) {
            const HeadPlan hp = head_plan(h->frozen.data(), h->n, pp.prefix_q, pp.prefix_len, h->N / 2);
            if (hp.phi_h > 0 && hp.window >= kHeadMinWindow) rc = h->d_head_rec.ensure((size_t)B * hp.record_words());
        }
    }
    hipError_t e = hipDeviceSynchronize();
    llr.release(); out.release(); pm.release();
    if (!rc && e != hipSuccess) return fail(POLAR_E_DEVICE, "polar_reserve: %s", hipGetErrorString(e));
    return rc;
}

int polar_count_errors_dev(polar_code_t *h, const uint8_t *d_a, const uint8_t *d_b, long B,
                           unsigned long long *d_err_count, void *stream) {
    int rc = check_args(h && d_a && d_b && d_err_count, kNoList, B);
    if (rc || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    HIP_TRY(polar_launch_count_errors(d_a, d_b, B, h->K, d_err_count, nullptr, (hipStream_t)stream));
    return POLAR_OK;
}

}  // extern "C"
