// polar_kernels.h — launch interface between the C-ABI host code and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

// element formats of the caller's channel LLR rows (the values of include/polar_amd.h)
#ifndef POLAR_LLR_F64
#define POLAR_LLR_F64  0
#define POLAR_LLR_F32  1
#define POLAR_LLR_F16  2
#define POLAR_LLR_BF16 3
#endif
static inline size_t polar_llr_esz(int fmt) { return fmt == POLAR_LLR_F64 ? 8 : fmt == POLAR_LLR_F32 ? 4 : 2; }
// blocks of a launch of one wave per row: a block for every row up to 8192, the waves loop over the rest
static inline int polar_rows_grid(long B) { return (int)(B < 8192 ? (B > 0 ? B : 1) : 8192); }
// before a launch with more dynamic LDS than the 48 KiB every kernel may have: ask for it (per launch: the attribute belongs to the
// function on the current device)
static inline hipError_t polar_allow_lds(const void *kernel, size_t lds) {
    return lds > 48 * 1024 ? hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
}

struct PolarDecodeParams {
    int n, N, K, crc, L;
    int W;                       // 32-bit words of decision history = ceil((K+crc)/32)
    int prefix_q, prefix_len;    // all-frozen prefix handled cooperatively: block size Q (0 = off), leaves Pe
    long B;                      // codewords
    const double *llr;           // [B][N] device (LLR mode: llr; probability mode: p1); elements of llr_fmt
    int llr_fmt;                 // element format of the channel LLRs (POLAR_LLR_*; the narrow ones are widened exactly in the load)
    const double *p0;            // [B][N] device (probability mode only)
    uint8_t *out;                // [B][K] device
    double *pm_out;              // [B] device or nullptr
    const uint8_t *frozen;       // [N] device
    const uint32_t *ctl;         // [N] device: per-leaf control word of the LLR kernel = frozen | zb << 1 | weak << 8, zb = log2 size (0, 2 or 3) of the all-frozen aligned block starting at this leaf, weak = unfrozen leaf in one of the worst channels (scalar-loaded); bits 9-10: rb = log2 size (0, 2 or 3) of the marked rate-1 block starting at this leaf (polar_handle.cpp; read by the list-of-32 units, polar_scl_leaf.inc — absent under the knob no_r1)
    unsigned int *work;          // device counter (zeroed before the launch): dynamic hand-out of codeword groups after a wave's first one
    const uint16_t *info_rank;   // [K+crc] device: rank of order[beta] among the unfrozen positions
    const uint32_t *crc_mask;    // [crc][W] device: parity masks over unfrozen ranks (check bit included)
    const double *tabs;          // [322] device: T[64] = 2^(-j/64), RC[129] = 1/(1+j/128), LC[129] = log(1+j/128)
    const double *pre;           // [B][N - Q + 1] device: prefix_kernel output (metric + node-0 f-chain), nullptr if off
    double *llr_scr;             // per-wave scratch: [grid][N - 2*SL][64]
    uint32_t *c_scr;             // per-wave scratch: [grid][2][N/32 - 2][64]
    uint32_t *hist_scr;          // per-wave scratch: [grid][W][64]
    // exp-domain fast path + fallback pass
    uint8_t *flags;              // [B] device (ED kernels): 1 = decode this codeword again with the LLR-domain kernel
    const uint32_t *cw_list;     // work list of codeword indices (fallback pass), nullptr = 0..B-1
    const unsigned int *cw_count;// device: number of entries of cw_list (read by the kernel), nullptr = B
    const unsigned int *n_dev;   // device: only the first min(B, *n_dev) codewords exist (Monte-Carlo alive lists), nullptr = B
    double *tab_scr;             // table mode (GS = 32, exp-domain): per-wave [grid][2][3N] layer-1/-2 value tables, nullptr = off
    uint32_t *var_scr;           //   per-wave [grid][N/32][64] variant nibbles of the paths
};
// The list-output launch (polar_launch_decode_llr_list) takes the decode parameters with the list's output pointers BEHIND them: every
// field above keeps its offset, and the kernels of the other translation units keep their argument block — and with it the
// offsets of the launch geometry the runtime appends to it, i.e. their machine code — byte for byte. `out` and `pm_out` are not
// written by that launch. Rows in the order of include/polar_amd.h polar_decode_scl_llr_list_batch_dev.
struct PolarListParams : PolarDecodeParams {
    uint8_t *list_cand;          // [B][L][K] device
    double *list_pm;             // [B][L] device or nullptr
    uint8_t *list_crc;           // [B][L] device or nullptr
    int32_t *list_nact;          // [B] device or nullptr
    int32_t *list_win;           // [B] device or nullptr
};

// The adaptive decode (polar_launch_decode_llr_adapt) takes the decode parameters with its own fields BEHIND them, for
// the same reason. One launch is one STAGE of a schedule of list sizes: a codeword whose winner is an active path that passes the CRC,
// or any codeword of the last stage, is delivered (`out`, `pm_out`, ad_stage, ad_crc); every decoded codeword gets its retry byte.
struct PolarAdaptParams : PolarDecodeParams {
    uint8_t *ad_retry;           // [B] device: 1 = decode this codeword again at the next list size, 0 = delivered; written for EVERY decoded codeword
    uint8_t *ad_stage;           // [B] device or nullptr: the stage that delivered the codeword
    uint8_t *ad_crc;             // [B] device or nullptr: 1 = the delivered word's path passed the CRC
    int ad_s, ad_last;           // this stage's index; 1 = last stage (deliver whatever the winner is)
};

// The two-phase list decode (polar_head_plan.h) takes the decode parameters with the hand-over BEHIND them, like the list output:
// the kernels of the other translation units keep their argument block. Phase A (polar_launch_decode_head_export: the groups of
// 4 lanes, L = 4) decodes the leaves up to head_phi and writes the records, phase B (polar_launch_decode_head_import: the list of
// 32) starts there. Same scratch, same geometry; each phase has its own work counter.
struct PolarHeadParams : PolarDecodeParams {
    unsigned long long *head_rec; // [B][head_rows][4] device: HeadPlan's record
    int head_phi, head_t, head_rows;
    uint32_t head_llr_mask, head_c_mask;
};
hipError_t polar_launch_decode_head_export(const PolarHeadParams &p, int grid, hipStream_t st);
hipError_t polar_launch_decode_head_import(const PolarHeadParams &p, int grid, hipStream_t st);

// launch geometry of scl_decode_llr_kernel: waves per block, LDS per block, and what a path column keeps in the per-wave scratch —
// the elements of the layers above 2^lds_log, the words of the big partial-sum layers (S >= 64)
static inline int polar_decode_waves_per_block(int pipe) { return pipe ? 1 : 4; }
static inline size_t polar_decode_lds_bytes(int lds_log, int pipe) {
    return 324 * 8 + (size_t)polar_decode_waves_per_block(pipe) * ((size_t)((2u << lds_log) - 1) * 64 * 8 + 128 * 8 + 128);
}
static inline size_t polar_decode_big(int N, int lds_log) { return N > (2 << lds_log) ? (size_t)(N - (2 << lds_log)) : 0; }
static inline size_t polar_decode_cwords(int N) { return N >= 128 ? (size_t)(N / 32 - 2) : 0; }
hipError_t polar_launch_prefix(const PolarDecodeParams &p, bool ed, double *ech_out, hipStream_t st);
hipError_t polar_launch_prefix_ed0(const PolarDecodeParams &p, double *ech_out, hipStream_t st);
hipError_t polar_launch_prefix_ed1(const PolarDecodeParams &p, double *ech_out, hipStream_t st);
int polar_prefix_is_staged(int N);
hipError_t polar_launch_decode_llr_ed0(const PolarDecodeParams &p, int gs, int lds_log, int pipe, int grid, hipStream_t st);
hipError_t polar_launch_decode_llr_ed1(const PolarDecodeParams &p, int gs, int lds_log, int pipe, int grid, hipStream_t st);
// one codeword per wave, state in LDS (the latency form; list sizes 2 .. 8 while polar_decode_lat_lds_bytes() fits 160 KiB)
hipError_t polar_launch_decode_lat(const PolarDecodeParams &p, int gs, bool ed, int blocks, hipStream_t st);
size_t polar_decode_lat_lds_bytes(int N, int gs, int W);
hipError_t polar_launch_decode_llr(const PolarDecodeParams &p, int gs, int lds_log, int pipe, int grid, bool ed, hipStream_t st);
// every surviving path of every codeword (LLR-domain arithmetic, batch geometry, default tuning: LDS_LOG = 3, four waves per block)
hipError_t polar_launch_decode_llr_list(const PolarListParams &p, int gs, int grid, hipStream_t st);
// one stage of the adaptive decode (LLR-domain arithmetic, batch geometry, default tuning), over rows 0 .. B-1 or the work list of p
hipError_t polar_launch_decode_llr_adapt(const PolarAdaptParams &p, int gs, int grid, hipStream_t st);
hipError_t polar_launch_ed_front(const void *llr, int llr_fmt, double *ech, uint8_t *flags, const double *tabs, int N, long B, const unsigned *n_dev, hipStream_t st);
hipError_t polar_launch_ed_collect(const uint8_t *flags, long B, const unsigned *n_dev, uint32_t *list, unsigned *count, hipStream_t st);

hipError_t polar_launch_decode_p1(const PolarDecodeParams &p, int gs, int grid, hipStream_t st);

struct PolarScP1Params {
    int n, N, K;
    long B;
    const double *p1;            // [B][N] device
    double *out;                 // [B][K] device (doubles, as MATLAB: 0.5 possible)
    const uint8_t *frozen;       // [N]
    const uint16_t *order;       // [N]
    double *scr;                 // per-wave scratch [grid][4*N][64]
};
hipError_t polar_launch_sc_p1(const PolarScP1Params &p, int grid, hipStream_t st);
// small batches: one codeword per wave, state in LDS (polar_sc_p1_lat_lds_bytes(N) must fit the device's LDS)
hipError_t polar_launch_sc_p1_lat(const PolarScP1Params &p, int grid, hipStream_t st);
size_t polar_sc_p1_lat_lds_bytes(int N);

// list size 1: pruned successive cancellation (polar_kernels_sc.hip)
struct PolarScParams {
    int n, N, K;
    long B;
    const double *ech_t;         // [B][N] device: channel values, stored form, kernel element order (sc8_front_kernel); unused when `llr` is set
    const void *llr;             // nullptr, or [B][N] device: the caller's rows (elements of llr_fmt: POLAR_LLR_*), read IN PLACE by the two
    int llr_fmt;                 //   visits of the top layer (no front pass): polar_sc8_can_fold() says for which schedules
    uint8_t *out;                // [B][K] device
    const uint32_t *ops;         // [n_ops] device: schedule words = type | log2(S) << 3 | first leaf << 8
    int n_ops;                   //   type 0 F, 1 G, 3 all-unfrozen, 4 combine, 6 all-frozen bound
    const uint16_t *order;       // [N] device (the first K entries are read)
    const double *tabs;          // [322] device
    double *a_scr;               // per-wave scratch: the layers larger than the LDS-resident ones, polar_sc8_scratch_doubles_per_wave()
    unsigned int *flag_words;    // [ceil(B/32)] device, bit = codeword to be decoded again by the general kernel
    uint8_t *flag_bytes;         // nullptr, or [B] (sc_lat_kernel only): the same flag as a byte per codeword, WRITTEN for every codeword
                                 //   (the zero-copy host path reads it from pinned memory instead of copying the flag words back)
    unsigned int *work;          // device counter (zeroed before the launch) or nullptr
    const unsigned int *n_dev;   // device: only the first min(B, *n_dev) codewords exist, nullptr = B
};
// eight lanes per codeword (channel values permuted per codeword [B][N])
size_t polar_sc8_lds_bytes(int N);
int polar_sc8_waves_per_block();
int polar_sc8_waves_per_cu(int N);
size_t polar_sc8_scratch_doubles_per_wave(int N);
int polar_sc8_fold_min_log();            // smallest log2(block length) whose top-layer visits can read the caller's rows in place
int polar_sc8_min_global_log();          // log2 of the smallest HBM-resident layer of the list-size-1 kernel
hipError_t polar_launch_sc8_front(const void *llr, int llr_fmt, double *ech_p, unsigned int *flag_words, const double *tabs,
                                  int n, long B, const unsigned *n_dev, hipStream_t st);
hipError_t polar_launch_sc8_decode(const PolarScParams &p, int grid_waves, hipStream_t st);
// one codeword per wave, whole state in LDS: the latency form for small batches (N <= 2^polar_sc_lat_max_log())
size_t polar_sc_lat_lds_bytes(int N, int n_ops);
int polar_sc_lat_max_log();
hipError_t polar_launch_sc_lat(const PolarScParams &p, int blocks, hipStream_t st);
hipError_t polar_launch_sc_collect(const unsigned int *flag_words, long B, const unsigned *n_dev, uint32_t *list, unsigned *count, hipStream_t st);

// Monte-Carlo code construction (polar_construct.hip)
struct PolarConstructParams {
    int n, N;
    long B;                      // runs in this batch
    uint64_t seed, trial0;       // run b uses trial index trial0 + b
    int constellation;           // POLAR_CONST_*
    double sigma, n0, cnorm;
    double *p1;                  // [B][N] device: P(bit = 1) per position
    uint32_t *info;              // [B][ceil(N/32)] device: packed message bits
    double *y_scr;               // per-wave scratch [grid][N][64]
    uint8_t *x_scr;              // per-wave scratch [grid][2*N][64]
    unsigned long long *num_err; // [N] device accumulators
};
hipError_t polar_launch_mc_front(const PolarConstructParams &p, int grid, hipStream_t st);
hipError_t polar_launch_mc_genie(const PolarConstructParams &p, int grid, hipStream_t st);

struct PolarEncodeParams {
    int n, N, K, crc;
    long B;
    const uint8_t *info;         // [B][K] device (encode) — unused by synth
    uint8_t *coded;              // [B][N] device (encode) — optional for synth
    const uint16_t *order;       // [N] device
    const uint8_t *crcm;         // [crc][K] device
    // synth
    uint64_t seed, trial0;
    long stride;                 // trial index = trial0 + b*stride, or sel[b] when sel != nullptr
    const uint64_t *sel;
    double s;
    int constellation;           // 0 = BPSK (s), else POLAR_CONST_* (sigma, n0, cnorm)
    double sigma, n0, cnorm;
    long info_block_div;         // info bits keyed by trial / info_block_div (100 = reference's refresh, 1 = every run)
    double *llr;                 // [B][N]
    uint8_t *info_out;           // [B][K] or nullptr
    const unsigned int *n_dev;   // device: only the first min(B, *n_dev) rows exist (Monte-Carlo alive lists), nullptr = B
    double *y_out;               // [B][N / n_bits] or nullptr: the received symbols of the ASK / BICM workload; with llr == nullptr
                                 // the demapper is left out (polar_synth_bicm_sym_dev)
};
hipError_t polar_launch_encode(const PolarEncodeParams &p, hipStream_t st);
hipError_t polar_launch_synth(const PolarEncodeParams &p, hipStream_t st);   // BPSK or ASK/BICM by p.constellation
// rank_out[b] = smallest row r < n_active[b] of cand [B][L][K] whose K bytes equal info [B][K], or L (polar_channel.hip)
hipError_t polar_launch_list_find(const uint8_t *cand, const int32_t *n_active, const uint8_t *info, long B, int L, int K,
                                  int32_t *rank_out, hipStream_t st);
hipError_t polar_launch_count_errors(const uint8_t *a, const uint8_t *b, long B, int K,
                                     unsigned long long *err, uint8_t *mismatch_flags, hipStream_t st);
// Path metric of given words (polar_kernels_metric.hip; include/polar_amd.h polar_path_metric_batch_dev): one wave per (row, word)
struct PolarMetricParams {
    int n, N, K, crc, R;
    long B;
    const void *llr;             // [B][N] device, elements of llr_fmt (POLAR_LLR_*)
    int llr_fmt;
    const uint8_t *info;         // [B][R][K] device
    const uint16_t *order;       // [N] device
    const uint8_t *crcm;         // [crc][K] device
    const double *tabs;          // [322] device
    double *scr;                 // nullptr: the N doubles of a word in LDS (polar_metric_lds_bytes(n, 1) must fit); else [grid][N] device
    double *pm;                  // [B][R] device
};
size_t polar_metric_lds_bytes(int n, int in_lds);
hipError_t polar_launch_path_metric(const PolarMetricParams &p, int grid, hipStream_t st);
// The five counters of the list statistics (include/polar_amd.h POLAR_LS_*, polar_kernels_metric.hip): rows [0, min(B, *n_dev)) of a list
// output against the sent info [B][K] and the sent word's own metric pm_sent [B]; ctr[0..4] are ADDED to
hipError_t polar_launch_list_classify(const uint8_t *cand, const double *pm, const uint8_t *crc_ok, const int32_t *n_active,
                                      const int32_t *winner, const uint8_t *sent, const double *pm_sent, long B, int L, int K,
                                      const unsigned int *n_dev, unsigned long long *ctr, hipStream_t st);
// The counters of the adaptive sweep (include/polar_amd.h POLAR_AD_*, polar_kernels_adapt.hip): delivered words out [B][K] against the
// sent info [B][K]; ctr[0 .. 3 + n_s) are ADDED to
hipError_t polar_launch_adapt_classify(const uint8_t *out, const uint8_t *stage, const uint8_t *crc_ok, const uint8_t *sent, long B,
                                       int K, int n_s, unsigned long long *ctr, hipStream_t st);
// SC-Flip (polar_kernels_flip.hip; include/polar_amd.h polar_decode_sc_flip_batch_dev): one codeword per wave, the whole
// state in LDS (polar_flip_lds_bytes(N) must fit: N <= 2^polar_flip_max_log()). ops: the walk over the code tree without its all-frozen
// subtrees, a word = type | lam << 3 | arg << 8 with lam the layer of the node the step produces (COMBINE: of the children) and arg
// the left sibling's address residue (G), the parent's address residue (COMBINE), or for QUAD — a node of four leaves, layer n - 2 (PAIR: of two, the root of
// n = 1) — the first leaf's position | the leaves' frozen bits << 16
#define POLAR_FLIP_OP_F 0
#define POLAR_FLIP_OP_G 1
#define POLAR_FLIP_OP_PAIR 2
#define POLAR_FLIP_OP_COMBINE 3
#define POLAR_FLIP_OP_QUAD 4
struct PolarFlipParams {
    int n, N, K, crc, T;         // T: max_flips (the kernel clamps it to K + crc)
    long B;
    const void *llr;             // [B][N] device, elements of llr_fmt (POLAR_LLR_*)
    int llr_fmt;
    const uint32_t *ops;         // [n_ops] device
    int n_ops;
    const uint16_t *order;       // [N] device
    const uint8_t *crcm;         // [crc][K] device
    const double *tabs;          // [322] device
    uint8_t *out;                // [B][K] device
    uint8_t *crc_ok, *n_dec;     // [B] device or nullptr
    int32_t *flip;               // [B] device or nullptr
    int32_t *cand;               // [B][T] device or nullptr
    double *mag;                 // [B][T] device or nullptr
};
size_t polar_flip_lds_bytes(int N);
int polar_flip_max_log();
int polar_flip_grid_cap();       // most blocks of a launch; the waves loop over the rest of the rows
hipError_t polar_launch_sc_flip(const PolarFlipParams &p, int grid, hipStream_t st);
// The counters of the SC-Flip sweep (include/polar_amd.h POLAR_FL_*): delivered words out [B][K] against the sent info [B][K];
// ctr[0 .. POLAR_FL_N) are ADDED to
hipError_t polar_launch_flip_classify(const uint8_t *out, const uint8_t *crc_ok, const uint8_t *n_dec, const uint8_t *sent, long B, int K,
                                      unsigned long long *ctr, hipStream_t st);
// SCAN soft-output decoding (polar_kernels_scan.hip; include/polar_amd.h polar_decode_scan_batch_dev): one codeword per
// wave, the whole state in LDS (polar_scan_lds_bytes(n) must fit: n <= polar_scan_max_log()). ops: the walk over the code tree, a word
// = type | lam << 3 | v << 7 | kl << 23 | kr << 25 | wb << 27: LEFT / RIGHT produce the L of a child of layer lam of the parent v; UP
// the B of node v of layer lam; PAIR the leaf LLRs of node v of layer n - 1 and, with wb, its B. kl, kr: what the left and the right
// child (PAIR: leaf) are — MIXED (its B is stored), all FROZEN (B = +inf), all UNFROZEN (B = 0).
#define POLAR_SCAN_OP_LEFT 0
#define POLAR_SCAN_OP_RIGHT 1
#define POLAR_SCAN_OP_UP 2
#define POLAR_SCAN_OP_PAIR 3
#define POLAR_SCAN_KIND_MIXED 0
#define POLAR_SCAN_KIND_FROZEN 1
#define POLAR_SCAN_KIND_UNFROZEN 2
#define POLAR_SCAN_F_MINSUM 1    // (the values of include/polar_amd.h POLAR_SCAN_MINSUM, POLAR_SCAN_EARLY_STOP)
#define POLAR_SCAN_F_EARLY 2
struct PolarScanParams {
    int n, N, K, crc, iters, flags;
    long B;
    const void *llr;             // [B][N] device, elements of llr_fmt (POLAR_LLR_*)
    int llr_fmt;
    const uint32_t *ops;         // [n_ops] device
    int n_ops;
    const uint16_t *order;       // [N] device
    const uint8_t *crcm;         // [crc][K] device
    const double *tabs;          // [322] device (exact arithmetic only)
    uint8_t *out;                // [B][K] device
    double *info_llr;            // [B][K] device or nullptr
    double *ext;                 // [B][N] device or nullptr
    uint8_t *crc_ok, *n_iter;    // [B] device or nullptr
};
size_t polar_scan_lds_bytes(int n);
int polar_scan_max_log();
int polar_scan_grid_cap();       // most blocks of a launch; the waves loop over the rest of the rows
hipError_t polar_launch_scan(const PolarScanParams &p, int grid, hipStream_t st);
// The counters of the SCAN sweep (include/polar_amd.h POLAR_SN_*): decided words out [B][K] against the sent info [B][K];
// ctr[0 .. POLAR_SN_N) are ADDED to
hipError_t polar_launch_scan_classify(const uint8_t *out, const uint8_t *crc_ok, const uint8_t *n_iter, const uint8_t *sent, long B, int K,
                                      int has_crc, unsigned long long *ctr, hipStream_t st);
// Monte-Carlo round on the device (PolarCode.cpp:728-742, 758-769): alive[i] = t0 + i*stride, *n = T
hipError_t polar_launch_mc_init_alive(uint64_t *alive, unsigned *n, uint64_t t0, long stride, long T, hipStream_t st);
// rows [0, min(B, *n_in)): block error iff decoded != sent; ctr[0] += block errors, ctr[1] += differing bits
// (PolarM/PolarCode.m:836-840); the trials in error are appended to alive_out / *n_out (the others were decoded
// correctly and are "counted, not simulated" at the higher Eb/N0 points)
hipError_t polar_launch_mc_count_compact(const uint8_t *decoded, const uint8_t *sent, long B, int K,
                                         const uint64_t *alive_in, const unsigned *n_in, uint64_t *alive_out, unsigned *n_out,
                                         unsigned long long *ctr, hipStream_t st);

// BICM demapper on its own (polar_channel.hip; Constellation.m:123-144, include/polar_synth.h polar_synth_bicm_demap2): received
// symbols y [B][M], M = N / nb (floor) -> llr / p1 [B][N], position i*nb + j = label bit j of symbol i; the tail positions
// M*nb .. N-1 get llr = 0, p1 = 0.5 (as synth_kernel)
struct PolarDemapParams {
    int N, M, nb;
    long B;
    const void *y;               // [B][M] device, double or float
    int y_f32;                   // 1: y are floats (widened exactly in the load)
    double n0;
    double pt[16];               // polar_const_point(id, s) / polar_const_norm(id), symbol index order
    double *llr, *p1;            // [B][N] device; either may be nullptr
    const unsigned int *n_dev;   // device: only the first min(B, *n_dev) rows exist, nullptr = B
};
hipError_t polar_launch_bicm_demap(const PolarDemapParams &p, hipStream_t st);

// Multi-level coding receiver over set-partition (or Gray) ASK (polar_kernels_mlc.hip, include/polar_synth.h):
// nb component codes of length M = N / nb = 2^m, component k = message positions k*M .. (k+1)*M - 1 (layer-major)
struct PolarMlcParams {
    int n, N, K, m, M, nb;
    long B;
    int constellation;           // POLAR_CONST_* (the receiver flag removed)
    double sigma, n0, cnorm;
    // front: trial of row b = sel[b] (alive lists) or trial0 + b*stride; info keyed by trial / info_block_div
    uint64_t seed, trial0;
    long stride, info_block_div;
    const uint64_t *sel;
    const unsigned int *n_dev;   // device: only the first min(B, *n_dev) rows exist, nullptr = B
    const uint8_t *info;         // [B][K] device: given info bits (encode), nullptr = drawn from the sweep's info stream
    uint8_t *info_out;           // [B][K] or nullptr
    uint8_t *coded;              // [B][N] or nullptr: coded bits in modulation order (symbol i, label bit k at i*nb + k)
    double *y;                   // [B][M] received symbols (front: written; decoders: read)
    const uint8_t *frozen;       // [N]
    const uint16_t *order;       // [N] (the first K entries are read)
    double *out;                 // [B][K] doubles (decode_sc_p1 convention) or nullptr
    uint8_t *out_bytes;          // [B][K] or nullptr: 0 / 1 for a decision of exactly 0.0 / 1.0, 2 otherwise
    double *scr;                 // lane-per-codeword decoder: per-wave scratch [grid][polar_mlc_scr_doubles(N, nb) / 64][64]
    // construction (genie): message bits packed [B][ceil(N/32)], per-position error counters [N] (layer-major)
    uint32_t *minfo;
    unsigned long long *num_err;
    uint8_t *x_scr;              //   per-wave scratch [grid][2*M + (nb-1)*M][64] bytes
};
size_t polar_mlc_scr_doubles(int N, int nb);
size_t polar_mlc_lat_lds_bytes(int N, int nb);
hipError_t polar_launch_mlc_front(const PolarMlcParams &p, int mode, hipStream_t st);   // mode 0: sweep / encode, 1: construction
hipError_t polar_launch_mlc_sc(const PolarMlcParams &p, int grid, hipStream_t st);
hipError_t polar_launch_mlc_sc_lat(const PolarMlcParams &p, int grid, hipStream_t st);
hipError_t polar_launch_mlc_genie(const PolarMlcParams &p, int grid, hipStream_t st);

// Gaussian-approximation code construction (polar_kernels_ga.hip; PolarM/PolarCode.m:198-255, GaussianApproximation/,
// CapacityHelper/, Constellation.m:190-370). All fp64.
// Capacity integrals: one block per (SNR, bit / layer) over the grid y_k = -ymax + k*dy, k = 0 .. P-1; per-thread sums
// in k order, then a fixed LDS tree: the result depends on the grid alone.
#define POLAR_GA_THREADS 256
#define POLAR_GA_PHI_FWD 10002          // x = 0 : 0.01 : 100.01 (initialize_phi.m)
#define POLAR_GA_PHI_INV 100001         // bins of -log(phi), width 1e-3 over [0, 100]
#define POLAR_GA_BINS 801               // polarized capacity: u-LLR bins of width 0.25 over [-100, 100]
struct PolarGaGrid {
    double n0, ymax, dy;
    long P;
};
struct PolarGaCapParams {
    int kind;                    // 0 BICM (get_bicm_capacity), 1 MLC (get_mlc_capacity), 2 get_bpsk_cap
    int nb, ns;
    double pt[16];               // normalised constellation points, symbol index order
    const PolarGaGrid *grid;     // [n_snr]
    double *out;                 // [n_snr][nb] (kind 2: [n_snr])
};
hipError_t polar_launch_ga_capacity(const PolarGaCapParams &p, int n_snr, hipStream_t st);
// phi tables: fwd [POLAR_GA_PHI_FWD] doubles; inv [POLAR_GA_PHI_INV] bit patterns of the largest x of each bin (0 = none),
// x_k = k*dx for k = 0 .. nx-1
hipError_t polar_launch_ga_phi(double *fwd, unsigned long long *inv, double dx, long nx, hipStream_t st);
// polarized capacity: counts [n_snr][nb][POLAR_GA_BINS][2] (u-LLR bin, sent bit), ADDED to
struct PolarGaPolParams {
    int constellation, nb;
    double cnorm;
    const double *sigma, *n0;    // [n_snr]
    uint64_t seed, trial0;
    long num_sym;
    unsigned long long *counts;
};
hipError_t polar_launch_ga_polarized(const PolarGaPolParams &p, int n_snr, hipStream_t st);
// GA polarization + stable descending sort + BLER prefix sums, one block per design point
struct PolarGaConsParams {
    int m, M, nb, N;             // sub-block length M = 2^m = N / nb
    const double *mean_llr;      // [n_points][nb]
    const double *fwd;           // phi tables (see polar_launch_ga_phi)
    const unsigned long long *inv;
    double *scr;                 // [n_points][2][N]
    double *channels;            // [n_points][N]
    uint16_t *order;             // [n_points][N]
    double *prefix;              // [n_points][N]
};
hipError_t polar_launch_ga_construct(const PolarGaConsParams &p, int n_points, hipStream_t st);
