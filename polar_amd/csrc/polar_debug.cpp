// polar_debug.cpp — measurement and test hooks (include/polar_amd_debug.h; not part of the reference's surface and not
// declared by include/polar_amd.h). The product library carries the measurement knobs only; the fault-injection keys
// (fail_device, fail_collective, stall_device, stall_ms, share_device, force_workers) exist only in the library built with
// -DPOLAR_TEST_HOOKS (libpolar_amd_test.so, what the GPU tests of the failure protocol load).
#include "polar_multi.h"
#include "polar_amd_debug.h"
#ifdef POLAR_TEST_HOOKS
#include "polar_head_plan.h"
// (polar_kernels.hip, units 2 and 6 of the test library: the continuation counters of the unit's last launch)
hipError_t polar_r1_counts_read_ed32(unsigned long long *out);
hipError_t polar_r1_counts_read_head(unsigned long long *out);
#endif

extern "C" {

int polar_debug_weak_leaves(const polar_code_t *h) { return polar_get_weak_leaves(h); }

int polar_debug_set(polar_code_t *h, const char *key, long value) {
    if (!h || !key) return fail(POLAR_E_ARG, "NULL argument");
    polar_code::Knobs &k = h->knobs;
    const std::string s(key);
    if (s == "mode_override") { if (value < -1 || value > 2) return fail(POLAR_E_ARG, "mode_override must be -1 (none), 0, 1 or 2"); k.mode_override = (int)value; }
    else if (s == "sc_no_fold") k.sc_no_fold = value != 0;
    else if (s == "no_tables") k.no_tables = value != 0;
    else if (s == "no_head") k.no_head = value != 0;
    else if (s == "no_r1") k.no_r1 = value != 0;
    else if (s == "head_min_b") { if (value < 0) return fail(POLAR_E_ARG, "head_min_b must be >= 0 (0 = default)"); k.head_min_b = value; }
    else if (s == "no_fuse_front") k.no_fuse_front = value != 0;
    else if (s == "no_prefix") h->prefix_on = (value == 0);          // (the all-frozen prefix decoded leaf by leaf by the list kernel itself)
    // (the cached streams / communicators / worker threads of the last device list were built under the old setting)
    else if (s == "no_rccl") { k.no_rccl = value != 0; multi_release(h, false); }
    else if (s == "force_rccl") { k.force_rccl = value != 0; multi_release(h, false); }
#ifdef POLAR_TEST_HOOKS
    else if (s == "host_fail_alloc") k.host_fail_alloc = value;
    else if (s == "share_device") { k.share_device = value != 0; multi_release(h, false); }
    else if (s == "fail_device") k.fail_device = (int)value;
    else if (s == "fail_collective") k.fail_collective = (int)value;
#endif
    else if (s == "lat_max_b") k.lat_max_b = value;
    else if (s == "lat_grid") { if (value < 0) return fail(POLAR_E_ARG, "lat_grid must be >= 0 (0 = default)"); k.lat_grid = value; }
    else if (s == "lane_grid") { if (value < 0) return fail(POLAR_E_ARG, "lane_grid must be >= 0 (0 = default)"); k.lane_grid = value; }
    else if (s == "list_chunk_cw") { if (value < 0) return fail(POLAR_E_ARG, "list_chunk_cw must be >= 0"); k.list_chunk_cw = value; }
    else if (s == "host_pipe_min_bytes") k.host_pipe_min_bytes = value;
    else if (s == "host_chunk_bytes") k.host_chunk_bytes = value;
    else if (s == "host_lanes") { if (value < 0 || value > HostPipe::kMaxLanes) return fail(POLAR_E_ARG, "host_lanes must be 0 (default) or 1 .. %d", HostPipe::kMaxLanes); k.host_lanes = value; }
    else if (s == "host_ramp") k.host_ramp = value;
    else if (s == "host_prefault") { if (value < -1 || value > 16) return fail(POLAR_E_ARG, "host_prefault must be -1 (none), 0 (default) or 1 .. 16 threads"); k.host_prefault = value; }
    else if (s == "host_threads") { if (value < 0) return fail(POLAR_E_ARG, "host_threads must be >= 0"); k.host_threads = value; }
    else if (s == "multi_grace_s") { if (value < 0) return fail(POLAR_E_ARG, "multi_grace_s must be >= 0"); k.multi_grace_s = value; }
#ifdef POLAR_TEST_HOOKS
    else if (s == "force_workers") { k.force_workers = value != 0; multi_release(h, false); }
    else if (s == "stall_device") k.stall_device = (int)value;
    else if (s == "stall_ms") { if (value < 0) return fail(POLAR_E_ARG, "stall_ms must be >= 0"); k.stall_ms = value; }
#endif
    else if (s == "multi_timeout_s") { if (value < 0) return fail(POLAR_E_ARG, "multi_timeout_s must be >= 0 (0 = no watchdog)"); k.multi_timeout_s = value; }
    else return fail(POLAR_E_ARG, "polar_debug_set: unknown key '%s'", key);
    drop_clones(h);          // (the per-device contexts carry a copy of the knobs)
    return POLAR_OK;
}
// (measurement builds: the handle's alpha scratch, where instrumented kernels leave their counters)
void *polar_debug_scratch_ptr(polar_code_t *h) { return h ? (void *)h->d_llr_scr.p : nullptr; }
long polar_debug_get(const polar_code_t *h, const char *key) {
    if (!key) return -1;
    const std::string s(key);
    if (s == "allocs") return (long)g_allocs.load();
    if (s == "comm_inits") return (long)polar_debug_comm_inits();
    if (!h) return -1;
    if (s == "test_hooks") {
#ifdef POLAR_TEST_HOOKS
        return 1;
#else
        return 0;
#endif
    }
    if (s == "weak_leaves") return h->weak_leaves;
    if (s == "mode_override") return h->knobs.mode_override;
    if (s == "head_phi") return h->last_head_phi;
    if (s == "lat_waves") return h->last_lat_waves;
    if (s == "lane_waves") return h->last_lane_waves;
    if (s == "scan_grid_cap") return polar_scan_grid_cap();
#ifdef POLAR_TEST_HOOKS
    if (s == "head_check") {
        // The premise of the two-phase decode, checked on what the head really left: row 2 of every record of the handle's last
        // two-phase call is read back and held against the plan (head_record_ok: no path killed, the top lanes, t) -> the number of
        // codewords that break it; -2: the last call left no records to read.
        if (!h->last_head_phi || h->last_head_b <= 0 || !h->d_head_rec.p) return -2;
        int P = 0;
        while (P < h->N && h->frozen[P]) ++P;
        const int Q = P >= 256 ? 256 : (P < 33 ? 0 : (P < 64 ? 64 : (P < 128 ? 128 : 256)));        // (prefix_params, which also allocates)
        const HeadPlan hp = head_plan(h->frozen.data(), h->n, Q, std::min(P, Q), h->N / 2);
        if (hp.phi_h != h->last_head_phi) return -3;
        std::vector<unsigned long long> rows2((size_t)h->last_head_b * 4);
        const size_t pitch = hp.record_words() * sizeof(unsigned long long);
        if (hipMemcpy2D(rows2.data(), 32, h->d_head_rec.p + 2 * 4, pitch, 32, (size_t)h->last_head_b, hipMemcpyDeviceToHost) != hipSuccess) return -4;
        long bad = 0;
        for (long b = 0; b < h->last_head_b; ++b) {
            unsigned long long r[4];
            for (int a = 0; a < 4; ++a) r[a] = rows2[(size_t)b * 4 + a];
            bad += head_record_ok(hp, r) ? 0 : 1;
        }
        return bad;
    }
    if (s.compare(0, 3, "r1_") == 0) {
        // rate-1 quad continuations of the last list-of-32 launch (the unit the handle's last call took: the two-phase import or
        // the single-phase kernel): finished in one step / given up; tried / finished after a first leaf that took the ranking
        // path; second quads of octets tried / finished in the step of the first. The caller has synchronised the call's stream.
        static const char *const names[6] = {"r1_committed", "r1_discarded", "r1_rank_tried", "r1_rank_committed", "r1_chain_tried", "r1_chain_committed"};
        for (int i = 0; i < 6; ++i) {
            if (s != names[i]) continue;
            unsigned long long c[6] = {0, 0, 0, 0, 0, 0};
            if ((h->last_head_phi ? polar_r1_counts_read_head(c) : polar_r1_counts_read_ed32(c)) != hipSuccess) return -2;
            return (long)c[i];
        }
    }
#endif
    if (s == "last_rounds") return h->last_rounds;
    if (s == "last_round_max_per_device") return h->last_round_max_per_device;
    if (s == "worker_threads_started") return h->worker_threads_started;
    if (s.compare(0, 9, "round_us_") == 0) {        // wall time of the steps of the last get_bler_quick* call
        if (h->round_us.empty()) return 0;
        std::vector<long> v(h->round_us);
        if (s == "round_us_count") return (long)v.size();
        if (s == "round_us_first") return v.front();
        std::sort(v.begin(), v.end());
        if (s == "round_us_min") return v.front();
        if (s == "round_us_max") return v.back();
        if (s == "round_us_median") return v[v.size() / 2];
        return -1;
    }
    if (s == "multi_poisoned") return h->multi_poisoned ? 1 : 0;
    if (s == "host_chunks") return h->hpipe ? h->hpipe->last_chunks : 0;
    if (s == "host_chunk_cw") return h->hpipe ? h->hpipe->last_chunk_cw : 0;
    if (s == "host_lanes") return h->hpipe ? h->hpipe->last_lanes : 0;
    if (s == "host_threads") return h->hpipe ? h->hpipe->last_threads : 0;
    if (s == "host_us_copy_in") return h->hpipe ? h->hpipe->us_copy_in : 0;
    if (s == "host_us_wait") return h->hpipe ? h->hpipe->us_wait : 0;
    if (s == "host_us_copy_out") return h->hpipe ? h->hpipe->us_copy_out : 0;
    if (s == "host_us_total") return h->hpipe ? h->hpipe->us_total : 0;
    return -1;
}
int polar_debug_comm_inits(void) { return g_comm_inits.load(); }

// The work list of the last call's fallback pass, read back from the handle's own buffers (nothing is copied per decode: the call
// sites of fallback_pass leave the pointers, polar_decode.cpp). The count is capped by the call's batch: the list buffer holds
// at least that many entries.
long polar_debug_fallback_rows(polar_code_t *h, uint32_t *rows, long cap) {
    if (!h || !h->fb_count) return -1;
    DevGuard dg_;
    if (ensure_device(h, dg_)) return -1;
    hipError_t e = hipStreamSynchronize((hipStream_t)h->fb_stream);
    unsigned int count = 0;
    if (e == hipSuccess) e = hipMemcpy(&count, h->fb_count, sizeof count, hipMemcpyDeviceToHost);
    if (e == hipSuccess && (long)count > h->fb_b) return -(long)hipErrorInvalidValue - 1;          // (a count no collect kernel can leave)
    const long n = std::min<long>(count, cap);
    if (e == hipSuccess && rows && n > 0) e = hipMemcpy(rows, h->fb_list, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    return e == hipSuccess ? (long)count : -(long)e - 1;
}

// One of the two alive lists of the step-wise Monte-Carlo engine (polar_mc_batch*: mc_round_launch, polar_montecarlo.cpp) as the
// handle's last round left it: copies min(count, cap) trial indices (in no particular order) to `out` and returns the count.
// Reads only; the engine's calls have synchronised their stream before they return.
long polar_debug_mc_alive(polar_code_t *h, int which, uint64_t *out, long cap) {
    if (!h || which < 0 || which > 1 || !h->d_alive[which].p || !h->d_nalive.p) return -1;
    DevGuard dg_;
    if (ensure_device(h, dg_)) return -1;
    unsigned int count = 0;
    hipError_t e = hipMemcpy(&count, h->d_nalive.p + which, sizeof count, hipMemcpyDeviceToHost);
    if (e == hipSuccess && (size_t)count > h->d_alive[which].cap) return -(long)hipErrorInvalidValue - 1;      // (a count no round can leave)
    const long n = std::min<long>(count, cap);
    if (e == hipSuccess && out && n > 0) e = hipMemcpy(out, h->d_alive[which].p, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost);
    return e == hipSuccess ? (long)count : -(long)e - 1;
}

// The control words as they were uploaded (marked != 0: the array with the rate-1 block field, else the plain one): copies
// min(N, cap) words to `words`, returns N; below 0: -(1 + hipError_t). Both libraries.
long polar_debug_ctl_words(polar_code_t *h, uint32_t *words, long cap, int marked) {
    if (!h) return -1;
    DevGuard dg_;
    if (ensure_device(h, dg_)) return -1;
    const long n = std::min<long>(h->N, cap);
    if (words && n > 0) {
        const hipError_t e = hipMemcpy(words, marked ? h->d_ctl_r1.p : h->d_ctl.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return -(long)e - 1;
    }
    return h->N;
}

}  // extern "C"
