// polar_host.h — INTERNAL header of the host side of libpolar_amd.so (the C-ABI of include/polar_amd.h): the handle
// (`struct polar_code`), its device buffers, and the functions the translation units share.
//
//   polar_handle.cpp      construction (the reference's constructor work), tables, device upload, getters / setters
//   polar_decode.cpp      decode_scl_llr on the device: the family choice (choose_family), one launcher per kernel family behind
//                         decode_impl, the device-resident entry points, P1 paths, encoder; default_scratch (list output, adaptive)
//   polar_mlc.cpp         MLC receiver: checks, parameter fill, dispatch of the multistage SC kernels, its entry points
//   polar_hostpipe.cpp    host-pointer entry points: small-batch staging and the pipelined large-batch path
//   polar_list.cpp        list output of decode_scl_llr (every surviving path), polar_list_find_dev, path metric of given words,
//                         the list statistics of the sweep (polar_mc_batch_list)
//   polar_adaptive.cpp    adaptive list decoding: a schedule of list sizes, escalated until the CRC passes, and its sweep
//   polar_flip.cpp        SC-Flip: CRC-aided single-bit retries of SC decoding, and its sweep
//   polar_scan.cpp        SCAN: soft-output decoding by soft cancellation, and its sweep
//   polar_sys.cpp         systematic coding: its host tables, precode / message recovery / soft message outputs, its workload and sweep
//   polar_rm.cpp          rate matching: patterns, forced leaves, the handle's pattern and its inverse tables, select / recover, the
//                         rate-matched decode, workload and sweep, the GA construction from a start vector
//   polar_bicm.cpp        Constellation mirror: modulate, BICM demapper, decode from received symbols
//   polar_montecarlo.cpp  get_bler_quick: device-side rounds, the driver of the pipelined rounds, Monte-Carlo code construction;
//                         the walk the sweeps of the five decoder variants share (sweep_begin, sweep_cells, sweep_walk)
//   polar_mc_schedule.h   the schedule of the pipelined rounds alone (standard library only: tests/test_mc_schedule.py runs it on a CPU)
//   polar_multi.cpp       multi-device context: RCCL binding, worker threads, watchdog, per-device clones
//   polar_debug.cpp       measurement knobs (include/polar_amd_debug.h); fault injection only with -DPOLAR_TEST_HOOKS
// What the variants (list output / path metric, adaptive, SC-Flip, SCAN, systematic) share is below: the frame of an entry point
// (on_device), the checks (check_args, check_list_sizes), the schedules of the tree-walking kernels (LeafCount, ops_prepare), the
// sweep (sweep_chunk, sweep_rows and the walk). The device side of it: polar_wave_frame.h.
#pragma once
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <sched.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <numeric>
#include <string>
#include <vector>

#include "polar_amd.h"
#include "polar_kernels.h"
#include "polar_synth.h"

namespace polar_host {

extern thread_local std::string g_err;
int fail(int code, const char *fmt, ...);

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(POLAR_E_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

extern std::atomic<unsigned long> g_allocs;     // hipMalloc calls of the handles' scratch buffers so far (polar_debug_get "allocs")

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;   // elements
    int ensure(size_t n) {
        if (n <= cap) return POLAR_OK;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        ++g_allocs;
        hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
        if (e != hipSuccess) return fail(POLAR_E_NOMEM, "hipMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(e));
        cap = n;
        return POLAR_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

int usable_cpus();

// Copies between the caller's pageable memory and the pinned staging slots of the host-pointer decode path, spread
// over a few parked threads: one core moves ~10 GB/s, the PCIe link ~55 GB/s.
struct CopyPool {
    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable cv_job, cv_done;
    unsigned gen = 0;
    bool quit = false;
    char *dst = nullptr; const char *src = nullptr; size_t bytes = 0;
    std::atomic<size_t> next{0};
    int pending = 0;
    static constexpr size_t kSlice = (size_t)1 << 20;
    void work() {
        for (;;) {
            const size_t off = next.fetch_add(kSlice);
            if (off >= bytes) return;
            memcpy(dst + off, src + off, std::min(kSlice, bytes - off));
        }
    }
    void start(int n) {
        for (int i = 0; i < n; ++i)
            threads.emplace_back([this] {
                unsigned seen = 0;
                for (;;) {
                    {
                        std::unique_lock<std::mutex> lk(m);
                        cv_job.wait(lk, [&] { return quit || gen != seen; });
                        if (quit) return;
                        seen = gen;
                    }
                    work();
                    std::lock_guard<std::mutex> lk(m);
                    if (--pending == 0) cv_done.notify_all();
                }
            });
    }
    void copy(void *d, const void *s, size_t n) {          // (the calling thread takes its share)
        if (threads.empty() || n < 2 * kSlice) { memcpy(d, s, n); return; }
        {
            std::lock_guard<std::mutex> lk(m);
            dst = (char *)d; src = (const char *)s; bytes = n; next = 0; pending = (int)threads.size(); ++gen;
        }
        cv_job.notify_all();
        work();
        std::unique_lock<std::mutex> lk(m);
        cv_done.wait(lk, [&] { return pending == 0; });
    }
    ~CopyPool() {
        { std::lock_guard<std::mutex> lk(m); quit = true; }
        cv_job.notify_all();
        for (auto &t : threads) t.join();
    }
};

// The caller's result array is usually FRESH (a MEX gateway, a std::vector, numpy: memory the process has never touched):
// every 4-KiB page of it takes a page fault on its first store, and the stores are the result copies at the END of the
// pipeline, on the calling thread's critical path (measured, round 6, 64 MiB of small pages: 6 ms of result copies instead of
// 0.8 ms per call — tools/fresh_out_probe.py). A few parked threads fault the pages in (MADV_POPULATE_WRITE: the contents are
// not touched; kernels without it: a locked add of 0 to one byte per page, atomic against the result copies) while the first
// chunks are copied in and decoded. Pages that are already resident cost a page-table walk. Persistent: creating the threads
// per call costs more than they save on the short calls.
struct PrefaultPool {
    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable cv_job, cv_done;
    unsigned gen = 0;
    bool quit = false;
    uintptr_t lo = 0, hi = 0, pg = 4096;
    std::atomic<uintptr_t> next{0};
    int pending = 0;
    static constexpr uintptr_t kStep = (uintptr_t)2 << 20;      // (in pieces, in address order: the first result copies need the FIRST pages first)
    void work() {
        for (;;) {
            const uintptr_t q = next.fetch_add(kStep);
            if (q >= hi) return;
            const size_t len = (size_t)std::min(kStep, hi - q);
#ifdef MADV_POPULATE_WRITE
            if (madvise((void *)q, len, MADV_POPULATE_WRITE) == 0) continue;
#endif
            for (uintptr_t r = q; r < q + len; r += pg) __atomic_fetch_add((volatile unsigned char *)r, (unsigned char)0, __ATOMIC_RELAXED);
        }
    }
    void start_threads(int n) {
        pg = (uintptr_t)sysconf(_SC_PAGESIZE);
        for (int i = 0; i < n; ++i)
            threads.emplace_back([this] {
                unsigned seen = 0;
                for (;;) {
                    {
                        std::unique_lock<std::mutex> lk(m);
                        cv_job.wait(lk, [&] { return quit || gen != seen; });
                        if (quit) return;
                        seen = gen;
                    }
                    work();
                    std::lock_guard<std::mutex> lk(m);
                    if (--pending == 0) cv_done.notify_all();
                }
            });
    }
    // fault in [p, p + bytes) in the background; wait() before the memory may be handed back to the caller
    void start(void *p, size_t bytes) {
        const uintptr_t a = ((uintptr_t)p + pg - 1) & ~(pg - 1), b = ((uintptr_t)p + bytes) & ~(pg - 1);
        if (threads.empty() || b <= a + 64 * pg) return;
        {
            std::lock_guard<std::mutex> lk(m);
            lo = a; hi = b; next = a; pending = (int)threads.size(); ++gen;
        }
        cv_job.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> lk(m);
        cv_done.wait(lk, [&] { return pending == 0; });
    }
    ~PrefaultPool() {
        { std::lock_guard<std::mutex> lk(m); quit = true; }
        cv_job.notify_all();
        for (auto &t : threads) t.join();
    }
};

}  // namespace polar_host
using namespace polar_host;

// The pipelined host-pointer decode path (host_decode): a ring of pinned staging slots and device slots, one copy stream,
// two decode lanes (the handle itself and a private copy of its tables with its own scratch) on their own streams.
struct HostPipe {
    static constexpr int kMaxLanes = 8, kMaxSlots = kMaxLanes + 2;
    int R = 0;                               // ring slots in use (lanes + 2)
    hipStream_t copy = nullptr, lane[kMaxLanes] = {};
    hipEvent_t h2d[kMaxSlots] = {}, done[kMaxSlots] = {};
    void *pin_in[kMaxSlots] = {}; uint8_t *pin_out[kMaxSlots] = {};
    void *d_in[kMaxSlots] = {}; uint8_t *d_out[kMaxSlots] = {};
    size_t in_cap = 0, out_cap = 0;          // bytes per slot
    polar_code *ctx[kMaxLanes] = {};         // [0] unused (the handle itself); the others are owned, and dropped with the clones by every setter
    std::unique_ptr<CopyPool> pool;
    std::unique_ptr<PrefaultPool> prefault;  // (parked threads that fault the caller's fresh result pages in)
    // what the last pipelined call did (polar_debug_get "host_chunks", "host_chunk_cw", "host_lanes", "host_threads",
    // "host_us_copy_in" / "_wait" / "_copy_out" / "_total": where the calling thread spent its time)
    long last_chunks = 0, last_chunk_cw = 0, last_lanes = 0, last_threads = 0;
    long us_copy_in = 0, us_wait = 0, us_copy_out = 0, us_total = 0;
};

struct SysTables;
struct RmTables;

struct polar_code {
    int n = 0, N = 0, K = 0, crc = 0;
    double eps = 0.0;
    std::vector<uint8_t> frozen;     // [N]
    std::vector<uint16_t> order;     // [N]
    std::vector<uint16_t> bitrev;    // [N]
    std::vector<uint8_t> crcm;       // [crc*K]
    // derived
    int W = 0;
    std::vector<uint16_t> info_rank; // [K+crc]
    std::vector<uint32_t> crc_mask;  // [crc*W]
    std::vector<uint8_t> sched;      // [N] rate-0 block schedule for the kernel (0 / 2 / 3)
    std::vector<uint32_t> ctl;       // [N] frozen | sched << 1 | weak-unfrozen-leaf << 8
    std::vector<uint32_t> ctl_r1;    // [N] the same | rate-1 block log2 size << 9 (derive_tables)
    int weak_leaves = 0;             // unfrozen leaves no construction for an ordinary channel would leave unfrozen (derive_tables)
    std::vector<uint32_t> sc_ops;    // schedule of the list-size-1 kernel (PolarScParams::ops)
    std::vector<uint32_t> sc_lat_ops;//   the same for its one-codeword-per-wave form: no folded F steps, mixed nodes of size 8 as ONE op (type 7)
    bool sc_fold = false;            //   its top-layer visits read the caller's rows in place (derive_tables)
    // device
    bool dev_ready = false;
    int device = -1, num_cu = 0;
    size_t lds_per_block = 0;        // hipDeviceAttributeMaxSharedMemoryPerBlock (160 KiB on gfx950): what the one-codeword-per-wave kernels are gated on
    DevBuf<uint8_t> d_frozen, d_crcm;
    DevBuf<uint16_t> d_order, d_info_rank;
    DevBuf<uint32_t> d_crc_mask, d_ctl, d_ctl_r1, d_sc_ops, d_sc_lat_ops, d_var_scr;
    DevBuf<double> d_tab_scr;
    DevBuf<unsigned long long> d_head_rec;   // two-phase list of 32: the hand-over records [B][rows][4] (polar_head_plan.h)
    int last_head_phi = 0;           //   hand-over leaf of the last decode_scl_llr call, 0 = one phase (polar_debug_get "head_phi")
    long last_head_b = 0;            //   ... and how many records it left (0: rows alive on the device only, Monte-Carlo): polar_debug_get "head_check"
    long last_lat_waves = 0;         // blocks of the last one-codeword-per-wave launch of the last decode call, 0 = it took none (polar_debug_get "lat_waves")
    long last_lane_waves = 0;        // blocks of the last codeword-per-lane launch sized by grid_that_fits (decode_scl_p1 / decode_sc_p1 / decode_mlc), 0 = the last call had none (polar_debug_get "lane_waves")
    // the work list the last decode_impl call handed to fallback_pass (polar_debug_fallback_rows): device pointers into the handle's
    // own buffers, the call's stream and batch; fb_count == nullptr: the last call had no fallback pass
    const unsigned int *fb_count = nullptr;
    const uint32_t *fb_list = nullptr;
    void *fb_stream = nullptr;
    long fb_b = 0;
    void note_fallback(const unsigned int *count, const uint32_t *list, void *st, long B) { fb_count = count; fb_list = list; fb_stream = st; fb_b = B; }
    DevBuf<unsigned int> d_flag_words;
    DevBuf<double> d_llr_scr, d_tabs, d_pre;
    DevBuf<uint32_t> d_c_scr, d_hist_scr;
    // staging for the host-pointer entry points
    DevBuf<double> d_in;
    DevBuf<float> d_f32;
    DevBuf<uint8_t> d_out, d_bytes_a, d_bytes_b;
    DevBuf<unsigned long long> d_counter;
    DevBuf<unsigned int> d_work;
    DevBuf<uint64_t> d_sel;
    // exp-domain fast path: stored-form channel values, guard flags, fallback work list + its length
    DevBuf<double> d_ech;
    DevBuf<uint8_t> d_flags;
    DevBuf<uint32_t> d_list;
    DevBuf<unsigned int> d_count;
    DevBuf<double> d_list_out;       // host-pointer list call: one chunk of list output (metrics, counts, winners, bits, CRC flags: polar_list.cpp)
    DevBuf<double> d_metric_scr;     // path metric of given words: the per-wave rows [grid][N] of the codes too long for LDS, and the sweep's sent-word metrics (polar_list.cpp)
    DevBuf<unsigned int> d_adapt_ctl;// adaptive decode: the work counters and list lengths of its stages, zeroed by one memset per call (polar_adaptive.cpp)
    std::vector<uint32_t> flip_ops;  // SC-Flip: the walk of sc_flip_kernel (PolarFlipParams::ops), built and uploaded by the first call (polar_flip.cpp)
    DevBuf<uint32_t> d_flip_ops;
    DevBuf<int32_t> d_flip_i32;      //   host form and sweep: flip [B] and cand [B][T]
    std::vector<uint32_t> scan_ops;  // SCAN: the walk of scan_kernel (PolarScanParams::ops), built and uploaded by the first call (polar_scan.cpp)
    DevBuf<uint32_t> d_scan_ops;
    SysTables *sys = nullptr;        // systematic coding: host tables, their device copies and staging, built by the first systematic call and dropped by polar_set_crc_matrix (polar_sys.cpp)
    RmTables *rm = nullptr;          // rate matching: the pattern set by polar_set_rate_match, its inverse tables, their device copies and scratch (polar_rm.cpp)
    DevBuf<double> d_bicm_llr;       // symbol-domain BICM receiver: the demapped LLR rows [B][N] that decode_impl reads (polar_bicm.cpp)
    int mode = 0;                    // 0 auto, 1 LLR-domain kernel only, 2 exp-domain kernel + fallback pass
    // Measurement / test knobs. The environment is read ONCE, when the handle is created (read_env_knobs): a decode never
    // calls getenv. The fault-injection and device-sharing hooks have no environment form at all: polar_debug_set() only.
    struct Knobs {
        int mode_override = -1;      // POLAR_MODE=<0|1|2>: replaces `mode`
        bool sc_no_fold = false;     // POLAR_SC_NO_FOLD: list size 1 decodes a permuted, converted copy (front pass)
        bool no_tables = false;      // POLAR_NO_TABLES: list of 17..32 without the layer-1/2 value tables
        bool no_head = false;        // POLAR_NO_HEAD: list of 17..32 in one phase (no 4-lane head, polar_head_plan.h)
        bool no_r1 = false;          // POLAR_NO_R1: control words without the rate-1 block field (every leaf of such a block a loop step)
        long head_min_b = 0;         //   smallest batch that takes the head (0 = default: 16-codeword waves fill the device)
        bool no_fuse_front = false;  // (hook) exp-domain lists: separate conversion pass in front of the prefix kernel (the round-3 path)
        bool no_rccl = false;        // POLAR_NO_RCCL: multi-device counters summed on the host
        bool force_rccl = false;     // POLAR_FORCE_RCCL: RCCL even with one device
        bool share_device = false;   // (test hook) one GPU may be listed several times: separate contexts, host-side sum
        int fail_device = -1;        // (test hook) this worker reports a failure in its second round, before the collective
        int fail_collective = -1;    // (test hook) this worker's collective enqueue "fails" in its second round (after the barrier)
        long multi_timeout_s = 1800; // watchdog of a multi-device round: communicators are aborted when a round takes longer
        long multi_grace_s = 10;     //   ... and how long each of its two further steps waits for the workers (MultiCtx::run_all)
        bool force_workers = false;  // (test hook) worker threads (and so the watchdog) even with one device
        int stall_device = -1;       // (test hook) this worker sleeps stall_ms in its second round before it launches anything
        long stall_ms = 0;
        long lat_max_b = 0;          // batches up to this size take the one-codeword-per-wave kernels (0 = default, -1 = never)
        // the pipelined host-pointer path (host_decode): 0 = default everywhere
        long host_pipe_min_bytes = 0;  // input bytes from which a host-pointer batch is pipelined (-1 = never: one copy in, decode, one copy out)
        long host_chunk_bytes = 0;     // input bytes per chunk / staging slot
        long host_lanes = 0;           // decode lanes (1 or 2)
        long host_threads = 0;         // threads that copy between the caller's memory and the pinned slots (calling thread included)
        long host_ramp = 0;            // -1: no small first chunks (all chunks equal)
        long host_fail_alloc = 0;      // (test hook) the staging slot with this number (1-based) cannot be allocated
        long lat_grid = 0;           //   at most this many blocks in a launch of theirs (0 = default: what the device holds); they loop over the rest
        long lane_grid = 0;          // at most this many blocks in a launch sized by grid_that_fits (0 = default: 16 waves per CU); the waves loop over the rest
        long list_chunk_cw = 0;        // codewords per output chunk of the host-pointer list call (polar_list.cpp; 0 = default)
        long host_prefault = 0;        // threads that fault the caller's (fresh) output pages in while the first chunks decode (0 = default, -1 = none)
    } knobs;
    // Monte-Carlo engine (device side): alive lists (double-buffered), their lengths, per-round counters
    DevBuf<uint64_t> d_alive[2];
    DevBuf<unsigned int> d_nalive;           // [2]
    DevBuf<unsigned long long> d_mc_ctr;     // [n_L*n_e][2]: block errors, bit errors of the round
    // pipelined rounds (mc_step_launch): the alive lists of the rounds in flight — slot (list size, round mod slots), double-buffered —,
    // the lengths the device wrote, and their host copy
    struct McSlot { DevBuf<uint64_t> list[2]; int cur = 0; long cnt = 0; };
    std::vector<McSlot> mc_slots;
    DevBuf<unsigned int> d_slot_n;
    std::vector<unsigned int> h_slot_n;
    // per-device clones for polar_get_bler_quick_multi (owned by this handle)
    std::vector<polar_code *> clones;
    // streams + RCCL communicators of the last multi-device call, kept for the next one with the same device list
    // (an 8-rank ncclCommInitAll costs about as long as a short sweep runs)
    struct MultiCtx *multi = nullptr;
    bool multi_poisoned = false;     // a multi-device round never returned (MultiCtx::run_all step 3): no further multi-device calls
    bool ctx_stuck = false;          //   ... and the worker that never came back was working on THIS context: it computes nothing any more
    // zero-copy staging of the host-pointer entry points for the smallest batches (host_decode): pinned, device-mapped
    void *pin_in = nullptr, *pin_in_dev = nullptr;     // LLR rows
    uint8_t *pin_out = nullptr, *pin_out_dev = nullptr; // decoded bits [B][K] followed by one flag byte per codeword
    size_t pin_in_cap = 0, pin_out_cap = 0;
    uint8_t *lat_flag_bytes = nullptr;                  // (set around a decode_impl call by host_decode)
    struct HostPipe *hpipe = nullptr;                   // pipelined staging of the large host-pointer batches (host_decode)
    // statistics of the last get_bler_quick* call (polar_debug_get)
    long last_rounds = 0, last_round_max_per_device = 0, worker_threads_started = 0;
    std::vector<long> round_us;      //   wall time of every round of that call (polar_debug_get "round_us_min" / "_median" / "_max" / "_first")
    // tuning
    int waves_per_cu = 0, lds_log = 0, pipe = -1;
    bool prefix_on = true;
};

namespace polar_host {

// Every compute entry point runs on the handle's device (the one current at creation) and leaves the
// caller's current device as it found it.
struct DevGuard {
    int prev = -1;
    ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

inline int pow2ceil(int v) { int p = 1; while (p < v) p <<= 1; return p; }
// the POLAR_CONST_* ids (include/polar_synth.h): the range of the ASK constellations — BPSK's id lies inside it —, and the same without BPSK
inline bool is_ask_constellation(int c) { return c >= POLAR_CONST_ASK4_GRAY && c <= POLAR_CONST_ASK16_SP; }
inline bool is_ask_not_bpsk(int c) { return is_ask_constellation(c) && c != POLAR_CONST_BPSK; }
// noise of the ASK workloads at an SNR in dB (main_MC_CC_Comparison.m:88-92, PolarCode.m:170, Constellation.m:251); n0 = sigma^2
inline double sigma_of_snr_db(double snr_db) { return std::sqrt(1.0 / 2) * std::pow(10.0, -snr_db / 20); }

// polar_handle.cpp
int derive_tables(polar_code *h);
int ensure_device(polar_code *h, DevGuard &dg);
void drop_clones(polar_code *h);          // per-device contexts and extra decode lanes carry a copy of the settings: every setter drops them
template <typename T>
int upload(DevBuf<T> &d, const std::vector<T> &v) {
    size_t n = v.size() ? v.size() : 1;
    int rc = d.ensure(n);
    if (rc) return rc;
    if (v.size()) HIP_TRY(hipMemcpy(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return POLAR_OK;
}
// The frame of an entry point of the decoder variants (polar_list.cpp ... polar_sys.cpp) around what it does: rc = the result of its
// argument checks; an error or an empty batch ends it there, else body() runs with the handle's device current
template <typename Body>
int on_device(polar_code *h, int rc, long B, Body body) {
    if (rc || B == 0) return rc;
    DevGuard dg;
    if ((rc = ensure_device(h, dg))) return rc;
    return body();
}
// The host-pointer forms of the list output, the path metric and the adaptive decode: the caller's B rows of `fmt` staged in d_in
// (whole doubles), and n results copied back to dst + at where the caller asked for them (after the stream was waited for)
inline int stage_rows(polar_code *h, const void *rows, int fmt, long B) {
    const size_t bytes = (size_t)B * h->N * polar_llr_esz(fmt);
    if (int rc = h->d_in.ensure((bytes + 7) / 8)) return rc;
    HIP_TRY(hipMemcpy(h->d_in.p, rows, bytes, hipMemcpyHostToDevice));
    return POLAR_OK;
}
template <typename T>
int copy_back(T *dst, size_t at, const T *d_src, size_t n) {
    if (dst) HIP_TRY(hipMemcpy(dst + at, d_src, n * sizeof(T), hipMemcpyDeviceToHost));
    return POLAR_OK;
}
// blocks of a one-codeword-per-wave launch: the launch site's own grid under the "lat_grid" knob, remembered for "lat_waves"
inline int lat_grid(polar_code *h, long grid) {
    if (h->knobs.lat_grid > 0) grid = std::min<long>(grid, h->knobs.lat_grid);
    h->last_lat_waves = grid;
    return (int)grid;
}
// waves a codeword-per-lane launch asks grid_that_fits for: the launch site's own count under the "lane_grid" knob
inline long lane_grid(const polar_code *h, long want) {
    return h->knobs.lane_grid > 0 ? std::min<long>(want, h->knobs.lane_grid) : want;
}
// codewords per chunk of a call of T: the list_chunk_cw knob, or what `budget` bytes hold at `per` bytes a codeword
inline long chunk_len(const polar_code *h, long T, size_t budget, size_t per) {
    return std::min<long>(T, h->knobs.list_chunk_cw > 0 ? h->knobs.list_chunk_cw : std::max<long>(1, (long)(budget / per)));
}
// The argument checks the entry points share, in the order the ABI pins: the pointers (`ptrs_set`: none is null), `mid` (the entry
// point's own llr_fmt_check, bicm_check or mlc_check), the list size (kNoList: the call has none), the batch
constexpr int kNoList = 1;
inline int check_args(bool ptrs_set, int L, long B, const std::function<int()> &mid = nullptr) {
    if (!ptrs_set) return fail(POLAR_E_ARG, "NULL argument");
    if (int rc = mid ? mid() : POLAR_OK) return rc;
    if (L < 1 || L > POLAR_MAX_LIST) return fail(POLAR_E_ARG, "list size %d out of range [1, %d]", L, POLAR_MAX_LIST);
    return B < 0 ? fail(POLAR_E_ARG, "negative batch") : POLAR_OK;
}
// the list sizes of a sweep over several (polar_mc_batch_list, polar_mc_batch_sys)
inline int check_list_sizes(const uint8_t *L, int n_L) {
    for (int i = 0; i < n_L; ++i)
        if (L[i] < 1 || L[i] > POLAR_MAX_LIST) return fail(POLAR_E_ARG, "list size %d out of range", (int)L[i]);
    return POLAR_OK;
}
// What the schedule builders of the kernels that walk the code tree ask (flip_schedule, scan_schedule): the unfrozen leaves under
// node w of layer l, which covers the leaves [w << (n - l), (w + 1) << (n - l))
struct LeafCount {
    int n;
    std::vector<int> before;         // [N + 1] unfrozen leaves before position i
    explicit LeafCount(const polar_code *h) : n(h->n), before(h->N + 1, 0) {
        for (int i = 0; i < h->N; ++i) before[i + 1] = before[i] + (h->frozen[i] ? 0 : 1);
    }
    int under(int l, int w) const { return before[(w + 1) << (n - l)] - before[w << (n - l)]; }
};
// every buffer a launch of such a kernel needs, BEFORE it (the handle's device current): its `lds` bytes must fit (`msg` if not);
// the schedule is built and uploaded by the first call
inline int ops_prepare(polar_code *h, size_t lds, const char *msg, std::vector<uint32_t> &ops, DevBuf<uint32_t> &d_ops,
                       void (*schedule)(polar_code *)) {
    if (lds > h->lds_per_block) return fail(POLAR_E_UNSUPPORTED, "%s", msg);
    if (ops.empty()) schedule(h);
    return d_ops.p ? POLAR_OK : upload(d_ops, ops);
}
// What the per-wave state scratch of a launch may take: at most 24 GiB, and at most half of what the device has free plus what the
// handle already holds for it (a smaller or busy GPU runs fewer persistent waves instead of failing with POLAR_E_NOMEM)
inline size_t scratch_budget(const polar_code *h) {
    size_t budget = (size_t)24 << 30, free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, (free_b + h->d_llr_scr.cap * sizeof(double)) / 2);
    return std::max(budget, (size_t)64 << 20);
}
// the persistent grid of the P1 and MLC kernels: `want` waves, each with `per_wave` bytes of scratch — halved until the scratch is there
template <typename Ensure>
int grid_that_fits(const polar_code *h, long want, size_t per_wave, Ensure ensure, int *grid_out) {
    // (the budget is a driver query — hipMemGetInfo takes milliseconds: asked only when the scratch the handle holds is too small)
    long grid = want;
    if ((size_t)want * per_wave > h->d_llr_scr.cap * sizeof(double)) grid = std::max<long>(1, std::min<long>(want, (long)(scratch_budget(h) / per_wave)));
    for (;;) {
        const int rc = ensure((int)grid);
        if (rc != POLAR_E_NOMEM || grid <= 64) { *grid_out = (int)grid; return rc; }
        (void)hipGetLastError();
        grid /= 2;
    }
}

// polar_decode.cpp
// the kernel families of decode_scl_llr, and which one a call takes on this handle (no side effects)
enum class Family { Sc8, ScLat, ListLat, BatchLlr, BatchEd };
Family choose_family(const polar_code *h, long B, int L, bool want_pm);
// phase (the one-codeword-per-wave kernels only): 0 = everything; 1 = the decode kernel alone — the caller looks at the flags
// *deferred names (none: the fallback ran; d_flag_words + 4; d_flags) and runs phase 2, the fallback pass, only when one is set
enum class Deferred { None, FlagWords, FlagBytes };
int decode_impl(polar_code *h, const void *d_llr, int llr_fmt, long B, const unsigned int *n_dev, int L, uint8_t *d_out,
                double *d_pm, void *stream, void *ev_start, void *ev_stop, int phase = 0, Deferred *deferred = nullptr);
// Launch geometry of the batch kernel: G codewords (groups of gs lanes) per wave, `grid` waves in blocks of wpb, each with big * 64 doubles
// and 2 * cwords * 64 words of scratch. tuned: the handle's tuning and the small-batch rule; else the default. false: the LDS does not fit.
struct BatchGeometry { int gs, G, wpc, lds_log, pipe, wpb, grid; size_t big, cwords; };
bool batch_geometry(const polar_code *h, long B, int L, bool tuned, BatchGeometry &g);
int ensure_batch_scratch(polar_code *h, const BatchGeometry &g);          // d_llr_scr, d_c_scr, d_hist_scr for g.grid waves
// the scratch of n default-tuning launches that run one after the other and share it (the list output: one; the adaptive stages):
// sized for the largest grid; a device too full for it runs fewer persistent waves — every g[i].grid is cut to what fits
int default_scratch(polar_code *h, BatchGeometry *g, int n);
// the ONE place the decode parameters are filled (tables, scratch, work counter; no prefix, optional pointers null): a caller adds its own
void base_params(const polar_code *h, int L, long B, PolarDecodeParams &p);
// the all-frozen prefix the batch kernels leave to prefix_kernel for groups of `gs` lanes: p.prefix_q / prefix_len / pre (d_pre grown)
int prefix_params(polar_code *h, int gs, PolarDecodeParams &p);
// (polar_kernels.h repeats the POLAR_LLR_* codes of include/polar_amd.h for the translation units that do not see the public header)
static_assert(POLAR_LLR_F64 == 0 && POLAR_LLR_F32 == 1 && POLAR_LLR_F16 == 2 && POLAR_LLR_BF16 == 3, "POLAR_LLR_* codes");
int llr_fmt_check(int fmt, const void *rows);      // POLAR_E_ARG for an unknown POLAR_LLR_* code or 16-bit rows at an odd address (polar_hostpipe.cpp)
void fill_enc(const polar_code *h, PolarEncodeParams &p);
// polar_mlc.cpp — MLC receiver (polar_kernels_mlc.hip): *cid = the constellation without POLAR_RX_MLC, after the checks of include/polar_amd.h
int mlc_check(const polar_code *h, int constellation, int *cid);
void fill_mlc(const polar_code *h, int cid, double snr_db, PolarMlcParams &p);   // snr_db: sigma / n0 of the sweep's axis
int mlc_decode_launch(polar_code *h, int cid, const double *d_y, double n0, long B, const unsigned int *n_dev, double *d_out,
                      uint8_t *d_out_bytes, hipStream_t st);
// polar_bicm.cpp — symbol-domain BICM receiver
int bicm_check(int constellation, double n0);             // POLAR_E_ARG for an unknown id or an n0 that is not finite and > 0
void fill_demap(int cid, int N, double n0, PolarDemapParams &p);
// demap B rows of symbols on `st` into the context's own LLR buffer (grown on demand): *d_llr = what decode_impl reads
int bicm_front(polar_code *c, int cid, double n0, const void *d_y, int y_f32, long B, hipStream_t st, const double **d_llr);
// polar_montecarlo.cpp — the channel of a sweep point in synth_kernel's parameters: BPSK at an Eb/N0 (constellation 0) or ASK / BICM at an SNR, both in dB
void fill_channel(const polar_code *h, PolarEncodeParams &p, int constellation, double snr_point);
// The walk polar_mc_batch_list, polar_mc_batch_adaptive, polar_mc_batch_flip, polar_mc_batch_scan and polar_mc_batch_sys share. A cell:
// one enabled entry of the caller's [n_rows][n_e] grid — its point of the axis, its chunk length, its `width` counters at `ctr` in
// d_mc_ctr and in `stats`, its row: the entry of the caller's list-size vector (0 where the sweep has none)
struct Sweep { polar_code *h; int cid; uint64_t seed, t0; long T, stride; const double *axis; uint64_t *stats; DevGuard dg; };
struct SweepCell { int point; long chunk; size_t ctr; int width; int row; };
// the checks in the order the ABI pins (`ptrs_set`, "the `what` no MLC receiver", the constellation, `sizes_ok`, the caller's `own`);
// past them with T > 0 the handle's device is current while `sw` lives (T == 0: POLAR_OK, nothing to do)
int sweep_begin(Sweep &sw, polar_code *h, bool ptrs_set, const char *what, int constellation, uint64_t seed, uint64_t t0, long T,
                long stride, const double *axis, bool sizes_ok, uint64_t *stats, const std::function<int()> &own);
// trials per chunk of a sweep that takes `per` bytes a trial: 512 MiB of LLR rows and what belongs to them, or the knob of the list
// calls; and the walk's own buffers at that size: the LLR rows in d_in, the sent info in d_bytes_a
inline long sweep_chunk(const polar_code *h, long T, size_t per) { return chunk_len(h, T, (size_t)512 << 20, per); }
inline int sweep_rows(polar_code *h, long chunk) {
    if (int rc = h->d_in.ensure((size_t)chunk * h->N)) return rc;
    return h->d_bytes_a.ensure((size_t)chunk * h->K);
}
// the cells of the enabled entries of the [n_rows][n_e] grid, row by row: `width` counters each at width * (row * n_e + ie), chunks
// of chunk_of[row] trials
std::vector<SweepCell> sweep_cells(const uint8_t *enabled, int n_rows, int n_e, int width, const std::vector<long> &chunk_of);
using SweepBody = std::function<int(const SweepCell &, long, const PolarEncodeParams &)>;
// width * n_rows * n_e zeroed device counters; per cell and chunk of c trials: synth_kernel into d_in and d_bytes_a, then
// body(cell, c, p) — p: what synth_kernel was just launched with; the null stream, buffers sized by the caller —; at the end the
// cells' counters ADD to stats
int sweep_walk(Sweep &sw, const std::vector<SweepCell> &cells, int width, int n_rows, int n_e, const SweepBody &body);
// polar_sys.cpp — drops the systematic tables and their device buffers (polar_destroy, polar_set_crc_matrix)
void sys_release(polar_code *h);
// polar_rm.cpp — drops the rate-matching pattern and its device buffers (polar_destroy, polar_set_rate_match)
void rm_release(polar_code *h);
// polar_hostpipe.cpp
// rows that are received symbols instead of LLRs (polar_decode_bicm_batch*): M elements per row, demapped on the device
struct SymRows { int cid, M; double n0; };
int host_decode(polar_code *h, const void *rows, int rows_fmt, const SymRows *sym, long B, int L, uint8_t *out);
void hostpipe_release(polar_code *h);
// polar_multi.cpp
void multi_release(polar_code *h, bool abort_comms);
polar_code *copy_ctx(polar_code *h, int dev);            // a copy of the handle's tables and settings bound to `dev`; the caller owns it
polar_code *clone_on_device(polar_code *h, int dev, bool fresh = false);

}  // namespace polar_host
