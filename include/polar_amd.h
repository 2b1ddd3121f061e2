/* polar_amd.h — C-ABI of the MI355X-native polar SC/SCL decoder (drop-in boundary).
 *
 * The reference (tavildar/Polar) has no FFI: its boundary is the public surface of
 * `class PolarCode` (PolarC/PolarCode.h:19-34; MATLAB twin PolarM/PolarCode.m:59-93,
 * 266-322, 781-850).  Every entry point below replaces one member of that surface
 * (cited per function) with plain pointers and sizes, so that a MEX gateway, a cgo/ctypes
 * stub or the C++ header-only mirror in polar_amd/cpp/PolarCode.hpp can bind it
 * (INTEGRATION.md shows each binding).
 *
 * Conventions
 *   - all functions return 0 on success, a negative POLAR_E_* code otherwise (one positive, non-error status exists:
 *     POLAR_W_WEAK_LEAVES from polar_create_explicit);
 *     polar_last_error() returns a thread-local message. No exceptions cross the ABI.
 *   - the caller owns every buffer; the library never retains a pointer past the call.
 *   - "host" entry points take host pointers (H2D/D2H included); "_dev" entry points take
 *     device pointers resident in HBM plus a hipStream_t passed as void*.
 *   - LLR sign convention as the reference: llr = ln(p0/p1), positive => bit 0
 *     (PolarCode.cpp:752). Bits are one uint8_t per bit (0/1), as the reference.
 *   - a handle is bound to the HIP device that was current at creation (or, when none was visible
 *     then, at its first compute call); every entry point runs there and restores the caller's current
 *     device. Calls on one handle must be serialised by the caller (the reference object is not
 *     re-entrant either: PolarCode.h:56-68), and the asynchronous "_dev" calls of one handle must all be
 *     issued on ONE stream (or be ordered by the caller): they share the handle's device scratch.
 *     A "_dev" call may (re)allocate that scratch when the batch or list size grows, which synchronises
 *     the device once.
 *   - the decoders run ONLY on the GPU: without a usable HIP device they fail with
 *     POLAR_E_DEVICE. There is no CPU fallback in this library.
 */
#ifndef POLAR_AMD_H
#define POLAR_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POLAR_OK 0
#define POLAR_E_ARG (-1)      /* invalid argument (NULL, size, L out of range, ...) */
#define POLAR_E_DEVICE (-2)   /* no HIP device / HIP runtime error */
#define POLAR_E_NOMEM (-3)
#define POLAR_E_UNSUPPORTED (-4)
#define POLAR_W_WEAK_LEAVES 1 /* polar_create_explicit only: the handle is valid, but the table leaves unfrozen leaves in the
                                 worst synthetic channels (see polar_set_mode): bit-exactness with the reference is limited there */

#define POLAR_MAX_N_LOG2 15   /* reference: uint16_t _block_length (PolarCode.h:40) */
#define POLAR_MAX_LIST 64     /* reference loops forever for L > 127 (uint8_t, PolarCode.cpp:525) */
#define POLAR_MAX_CRC 32

typedef struct polar_code polar_code_t;

const char *polar_last_error(void);
/* library/ABI version: major*10000 + minor*100 + patch */
int polar_version(void);

/* ---- construction: PolarCode::PolarCode + create_bit_rev_order + initialize_frozen_bits
 *      (PolarCode.h:19-28, PolarCode.cpp:17-58, 647-656).
 * Bhattacharyya/BEC construction with design parameter `eps`; the info order is produced by
 * the same libstdc++ std::sort call as the reference, and — exactly like the reference — the
 * random-parity "CRC" matrix consumes crc*K draws of the process-global glibc rand() stream
 * (PolarCode.cpp:51-56).  Use polar_create_explicit() to pass every table yourself. */
int polar_create(int n, int K, double eps, int crc, polar_code_t **out);

/* Explicit tables (e.g. a Monte-Carlo constructed code, PolarM/PolarCode.m:111-135):
 * frozen[N] (1 = frozen), order[N] (= _channel_order_descending; only the first K+crc
 * entries are used), crc_matrix[crc*K] row-major (may be NULL when crc == 0). */
int polar_create_explicit(int n, int K, int crc, const uint8_t *frozen, const uint16_t *order,
                          const uint8_t *crc_matrix, polar_code_t **out);
void polar_destroy(polar_code_t *h);

/* table getters (PolarCode.h:45-48) */
int polar_get_params(const polar_code_t *h, int *n, int *N, int *K, int *crc);
int polar_get_frozen(const polar_code_t *h, uint8_t *frozen /*[N]*/);
int polar_get_order(const polar_code_t *h, uint16_t *order /*[N]*/);
int polar_get_bitrev(const polar_code_t *h, uint16_t *bitrev /*[N]*/);
int polar_get_crc_matrix(const polar_code_t *h, uint8_t *m /*[crc*K]*/);
int polar_set_crc_matrix(polar_code_t *h, const uint8_t *m /*[crc*K]*/);

/* ---- PolarCode::encode (PolarCode.cpp:60-91; PolarCode.m:266-276) ---- */
int polar_encode(polar_code_t *h, const uint8_t *info /*[K]*/, uint8_t *coded /*[N]*/);
int polar_encode_batch(polar_code_t *h, const uint8_t *info /*[B*K]*/, long B, uint8_t *coded /*[B*N]*/);
int polar_encode_batch_dev(polar_code_t *h, const uint8_t *d_info, long B, uint8_t *d_coded, void *stream);

/* ---- PolarCode::decode_scl_llr (PolarCode.cpp:130-148; PolarCode.m:312-322) ----
 * 1 <= L <= POLAR_MAX_LIST.  out[K] = decoded information bits in the reference's order
 * (Info[_channel_order_descending[beta]], PolarCode.cpp:172-174). */
int polar_decode_scl_llr(polar_code_t *h, const double *llr /*[N]*/, int L, uint8_t *out /*[K]*/);
/* batched, row-major, codeword-contiguous: llr[B*N] -> out[B*K].
 * Small batches — the reference's own loops decode one codeword per call (PolarCode.cpp:756,
 * PolarM/main_MC_CC_Comparison.m:96) — take latency kernels with ONE codeword per wave and the decoder state in LDS: list size 1
 * up to 2048 codewords (N <= 4096), list sizes 2 .. 8 up to one codeword per CU while the state fits 160 KiB of LDS (N = 2048: lists
 * up to 4; N = 1024: up to 8). Same bits as the batch kernels (tests/: every such test runs both). Batches of at most 64
 * codewords at list size 1 are staged in pinned, device-mapped host memory (no DMA copies).
 * Large batches (from 32 MiB of LLRs at L = 1, 1 GiB at L = 2, half a GiB or one full round of resident waves at L = 3 .. 8, half a GiB or two rounds for larger lists: below that one copy in, one launch and one copy out is faster) are PIPELINED inside the call: chunks are copied from the caller's (pageable) memory into
 * pinned slots by a few host threads, moved on a copy stream and decoded on two or three decode lanes with their own scratch
 * (the handle keeps slots, streams, lanes and threads: 0.3 - 1.3 GiB of pinned and device memory after the first such call):
 * min(device rate, PCIe rate) minus one decode launch, whatever the batch size; device memory use is bounded by the slots,
 * not by B. Same bits as one decode of the whole batch (tests/test_gpu_parity.py: chunk boundaries). */
int polar_decode_scl_llr_batch(polar_code_t *h, const double *llr, long B, int L, uint8_t *out);
/* device-resident: d_llr/d_out live in HBM; asynchronous on `stream` (hipStream_t).
 * d_pm (optional, may be NULL) receives the winning path metric per codeword. */
int polar_decode_scl_llr_batch_dev(polar_code_t *h, const double *d_llr, long B, int L, uint8_t *d_out,
                                   double *d_pm, void *stream);
/* single-precision LLRs at the boundary (half the PCIe / HBM input bytes): every float is widened
 * exactly to the reference's double on the device, so the result equals decode_scl_llr on
 * (double)llr[i]. Host-pointer and device-resident forms. */
int polar_decode_scl_llr_batch_f32(polar_code_t *h, const float *llr, long B, int L, uint8_t *out);
int polar_decode_scl_llr_batch_dev_f32(polar_code_t *h, const float *d_llr, long B, int L, uint8_t *d_out,
                                       double *d_pm, void *stream);
/* The same two calls for any element format of the channel LLRs. POLAR_LLR_F64 / _F32 are the entry points above (which forward
 * here); POLAR_LLR_F16 (IEEE binary16) and POLAR_LLR_BF16 (bfloat16) take raw 16-bit patterns — what a half / bfloat16
 * tensor or a numpy float16 array holds — at a quarter of the doubles' PCIe / HBM input bytes. The contract is the
 * float form's, word for word: out == decode_scl_llr(widen(llr)), bit for bit, widen = the exact value of the pattern as a
 * double (signed zeros, subnormals, +-inf and NaN patterns included: they behave as the same doubles behave). The widening
 * happens in the loads of the kernels that read the caller's rows (integer operations on the pattern: no denormal mode can
 * flush a subnormal); an aligned batch is never copied. Any other `fmt` is POLAR_E_ARG, before the device is touched; so are
 * 16-bit rows at an odd address. */
#define POLAR_LLR_F64  0
#define POLAR_LLR_F32  1
#define POLAR_LLR_F16  2
#define POLAR_LLR_BF16 3
int polar_decode_scl_llr_batch_fmt(polar_code_t *h, const void *llr, int fmt, long B, int L, uint8_t *out);
int polar_decode_scl_llr_batch_dev_fmt(polar_code_t *h, const void *d_llr, int fmt, long B, int L, uint8_t *d_out,
                                       double *d_pm, void *stream);
/* Pre-size the handle's device scratch for decodes of up to B codewords at list sizes 1 .. L (runs one decode per kernel
 * family on generated inputs — the list-size-1 kernel, the 2-lane groups, every power-of-two lane group up to L, with and
 * without d_pm — and waits for them). The device-resident entry points grow their scratch on demand — a hipFree/hipMalloc,
 * i.e. an implicit device synchronisation, whenever B or L exceeds anything seen before; after polar_reserve they do not
 * allocate for calls of at most B codewords and list size at most L, LLRs of any format (double, float, fp16, bf16), under the handle's current mode and
 * tuning (tests/test_gpu_parity.py and tests/test_gpu_llr16.py assert it on the allocation counter, polar_debug_get "allocs").
 * d_llr needs the natural alignment of its element type; rows that start 16-byte aligned (any hipMalloc'ed batch) let the
 * list-size-1 kernel read them in place, other pointers are decoded through a converted copy (same results). */
int polar_reserve(polar_code_t *h, long B, int L);
/* same, recording two hipEvent_t (may be NULL) on `stream` immediately around the launch of the
 * dominant kernel (scl_decode_llr_kernel), i.e. after the small all-frozen-prefix kernel — for
 * bench.py's roofline line */
int polar_decode_scl_llr_batch_dev_ev(polar_code_t *h, const double *d_llr, long B, int L, uint8_t *d_out,
                                      double *d_pm, void *stream, void *ev_start, void *ev_stop);

/* ---- list output of decode_scl_llr: every path the list decoder holds at the end of a codeword ----
 * (no member of the reference's class: its findMostProbablePath, PolarCode.cpp:609-644, returns one path and drops the rest.)
 * Per codeword, rows r = 0 .. L-1:
 *   cand[B][L][K]  uint8   information bits of the path in row r, in the reference's order (as `out` of decode_scl_llr)
 *   pm[B][L]       double  its path metric
 *   crc_ok[B][L]   uint8   1 = the path passes the handle's CRC (crc == 0: 1 for every active path)
 *   n_active[B]    int32   paths the decoder holds; fewer than L only when the list never filled (more entries than 2^K words)
 *   winner[B]      int32   the row decode_scl_llr returns for this codeword, or -1 where the reference returns its never-activated
 *                          path 0 (no candidate with a finite metric AND a list that never filled: the all-zero word)
 * Row order: CRC pass before fail, then the smaller metric (+inf last), then the lower path index of the decoder. Rows
 * n_active .. L-1 are padding: bits 0, pm = +inf, crc_ok = 0. Outside the degenerate rows just described winner is 0.
 * cand[b][winner[b]] (K zeros for -1) is bit for bit the `out` of polar_decode_scl_llr_batch_fmt for the same row, and
 * pm[b][winner[b]] bit for bit the d_pm of polar_decode_scl_llr_batch_dev_fmt under polar_set_mode(h, 1) with the batch kernel.
 * `fmt` = POLAR_LLR_*, with the alignment rules of polar_decode_scl_llr_batch_dev_fmt. 1 <= L <= POLAR_MAX_LIST, any value (the
 * decoder works on the next power of two of lanes). d_cand / cand is required, the other four outputs may be NULL. POLAR_E_ARG,
 * before the device is touched: unknown fmt, NULL handle / rows / cand, L out of range, negative B, 16-bit rows at an odd address;
 * B = 0 is POLAR_OK.
 * One kernel family serves every call: the LLR-domain batch kernel (mode 1's arithmetic) at its default tuning. polar_set_mode,
 * polar_set_tuning and the latency threshold do not affect a list call; there is no one-codeword-per-wave form, so a small batch
 * takes as long as a batch that fills the device once.
 *   _dev   device pointers, stream-ordered on `stream`, no host synchronisation: one prefix launch (where the code has an
 *          all-frozen prefix and L >= 3) and one decode launch. It grows the handle's scratch on demand like the other _dev calls;
 *          polar_reserve's no-allocation promise does NOT cover it (reserve sizes the scratch of decode_scl_llr's kernels only).
 *   host   host pointers: ONE copy of all B rows in, then per chunk of codewords the launches, a wait and the copies out. The
 *          chunk (256 MiB of list output: L K + 9 L + 8 bytes per codeword) bounds the device memory of the OUTPUT; the input is
 *          resident for the whole call. No pipelining, no pinned staging, no latency kernels: a convenience form.
 * polar_list_find_dev: d_rank[b] = the smallest row r < d_n_active[b] whose K bits equal d_info[b] ([B][K], e.g. the sent word),
 * or L when there is none — "was the sent word in the list?" without moving the list to the host. All pointers required. */
int polar_decode_scl_llr_list_batch_dev(polar_code_t *h, const void *d_llr, int fmt, long B, int L, uint8_t *d_cand, double *d_pm,
                                        uint8_t *d_crc_ok, int32_t *d_n_active, int32_t *d_winner, void *stream);
int polar_decode_scl_llr_list_batch(polar_code_t *h, const void *llr, int fmt, long B, int L, uint8_t *cand, double *pm,
                                    uint8_t *crc_ok, int32_t *n_active, int32_t *winner);
int polar_list_find_dev(polar_code_t *h, const uint8_t *d_cand, const int32_t *d_n_active, const uint8_t *d_info, long B, int L,
                        int32_t *d_rank, void *stream);

/* ---- error analysis of the list decoder: the metric of a given word, list-miss / undetected / ML-bound counters ----
 * polar_path_metric_batch[_dev]: SC along GIVEN decisions. For row b and word r, pm[b][r] is the metric the list decoder assigns to
 * the path whose information bits are info[b][r][0..K-1] (reference order, as `out` / `cand`), check bits = the handle's CRC matrix
 * applied to them, frozen bits 0. The R words of a row share its channel row llr[b]. Arithmetic: the LLR-domain list kernel's,
 * the N leaf terms added in decoding order in one fp64 chain — where the list output of the same row holds that word with
 * crc_ok = 1, pm equals the list's pm[b][row] BIT FOR BIT (a row with crc_ok = 0 decided other check bits: another path). A word
 * need not be in any list: the sent word's metric when the decoder lost it is what the ML bound below is made of.
 * `fmt` = POLAR_LLR_*, alignment rules of the list call; 1 <= R <= POLAR_MAX_LIST (the cand of a list call can be passed back with
 * R = L). POLAR_E_ARG before the device is touched: NULL pointers, unknown fmt, 16-bit rows at an odd address, R out of range,
 * negative B; B = 0 is POLAR_OK. _dev: device pointers, stream-ordered, no host synchronisation, one launch (one wave per word, its
 * N doubles in LDS up to N = 16384, beyond that in handle scratch grown on demand — polar_reserve does not cover it). Host form:
 * copies in, the launch, a wait, the copy out. */
int polar_path_metric_batch_dev(polar_code_t *h, const void *d_llr, int fmt, const uint8_t *d_info /*[B][R][K]*/, long B, int R,
                                double *d_pm /*[B][R]*/, void *stream);
int polar_path_metric_batch(polar_code_t *h, const void *llr, int fmt, const uint8_t *info, long B, int R, double *pm);
/* polar_mc_batch_list: like polar_mc_batch / polar_mc_batch_bicm for the trials {t0 + i*stride : i < T}, with the list decoder's end
 * state classified on the device. Every ENABLED (L, point) simulates all T trials (no "decoded at a lower Eb/N0 => not simulated":
 * the statistics are per point) and ADDS to stats[(li*n_e + ie)*POLAR_LS_N + c] (host uint64), c =
 *   POLAR_LS_RUN    every trial
 *   POLAR_LS_ERR    cand[winner] differs from the sent info (K zeros for winner -1): decode_scl_llr's block error
 *   POLAR_LS_MISS   no row r < n_active holds the sent info (polar_list_find_dev would return L): even a genie selector fails.
 *                   MISS <= ERR; ERR - MISS are the selection errors
 *   POLAR_LS_UNDET  ERR, winner >= 0 and crc_ok[winner] = 1: a wrong word delivered as valid (crc == 0: every error with a winner)
 *   POLAR_LS_ML     UNDET and pm[winner] <= the sent word's own metric (polar_path_metric_batch_dev): a valid word at least as
 *                   likely as the sent one exists, so an ML decoder of the concatenated code errs too — the lower bound on ML BLER
 * `constellation` 0 (or POLAR_CONST_BPSK): BPSK on the Eb/N0 axis; POLAR_CONST_ASK*: the BICM front end on the SNR axis. POLAR_RX_MLC,
 * NULL pointers, a list size out of range, negative T, stride < 1: POLAR_E_ARG before the device is touched; T = 0 is POLAR_OK and
 * leaves stats alone. The trials run in chunks (256 MiB of list output, or the "list_chunk_cw" knob), so T is not bounded by the
 * L K bytes per trial; the counters are read once, at the end of the call. */
#define POLAR_LS_RUN   0
#define POLAR_LS_ERR   1
#define POLAR_LS_MISS  2
#define POLAR_LS_UNDET 3
#define POLAR_LS_ML    4
#define POLAR_LS_N     5
int polar_mc_batch_list(polar_code_t *h, int constellation, uint64_t seed, uint64_t t0, long T, long stride,
                        const double *axis, int n_e, const uint8_t *L, int n_L, const uint8_t *enabled /*[n_L*n_e]*/,
                        uint64_t *stats /*[n_L*n_e][POLAR_LS_N]*/);

/* ---- adaptive list decoding: escalate the list size until the CRC passes (Li, Shen, Tse 2012) ----
 * (no member of the reference's class.) A schedule is n_s list sizes Ls[0] < Ls[1] < ... < Ls[n_s-1], 1 <= n_s <=
 * POLAR_AD_MAX_STAGES, each in 1 .. POLAR_MAX_LIST, any value (not only powers of two); a single entry is valid. Stage s decodes a
 * codeword with a list of Ls[s] and ACCEPTS it when the winner is an active path that itself passes the handle's CRC — in terms of
 * polar_decode_scl_llr_list_batch_dev at that list size: winner >= 0 && crc_ok[winner] == 1; the winner the reference takes when no
 * path passes is not accepted. Only codewords not accepted go on to stage s + 1. With s* = the first accepted stage, or n_s - 1:
 *   out[B][K]   uint8   information bits of the list-of-Ls[s*] decode: bit for bit cand[b][winner[b]] of the list call at that list
 *                       size, hence polar_decode_scl_llr_batch_fmt(.., Ls[s*]); K zeros for winner -1
 *   pm[B]       double  that winner's path metric, bit for bit the list call's pm[b][winner] (+inf for winner -1)
 *   stage[B]    uint8   s*
 *   crc_ok[B]   uint8   1 = stage s* accepted the word; 0 only at the last stage (always 0 for winner -1)
 * out / d_out is required, the other three outputs may be NULL. Arithmetic as the list call's: the LLR-domain batch kernel (mode 1's,
 * the reference's bits) at its default tuning; polar_set_mode, polar_set_tuning and the latency threshold do not affect it. A handle
 * with crc == 0 is refused (POLAR_E_ARG): there is nothing to accept on. POLAR_E_ARG, before the device is touched: NULL handle /
 * rows / out / schedule, n_s out of range, a size out of range, a schedule that is not strictly increasing, unknown fmt, 16-bit rows
 * at an odd address, negative B; B = 0 is POLAR_OK.
 *   _dev   device pointers (the schedule is a host array), stream-ordered on `stream`, no host synchronisation: one memset of a small
 *          control block, the prefix launch of stage 0 (where the code has an all-frozen prefix and Ls[0] >= 3), n_s decode launches
 *          and n_s - 1 launches between them that turn the retry flags into the next stage's work list. A later stage's grid is
 *          sized for B (the host never learns a count); its waves past the end of the list leave at once. Two calls on one handle
 *          and one stream need no synchronisation between them. It grows the handle's scratch on demand like the other _dev calls;
 *          polar_reserve's no-allocation promise does NOT cover it.
 *   host   host pointers: one copy of all B rows in, the _dev sequence, a wait, the copies out. No pipelining, no pinned staging:
 *          a convenience form like the list call's.
 * polar_mc_batch_adaptive: like polar_mc_batch_list for ONE schedule: every ENABLED point of `axis` simulates all the trials
 * {t0 + i*stride : i < T} and ADDS to stats[ie*(3 + n_s) + c] (host uint64), c =
 *   POLAR_AD_RUN         every trial
 *   POLAR_AD_ERR         the delivered word differs from the sent info
 *   POLAR_AD_UNDET       ERR and crc_ok = 1: a wrong word delivered as valid
 *   POLAR_AD_STAGE0 + s  trials delivered by stage s (they add up to RUN)
 * `constellation` as polar_mc_batch_list (BPSK on the Eb/N0 axis, POLAR_CONST_ASK*: the BICM front end on the SNR axis; POLAR_RX_MLC,
 * NULL pointers, a bad schedule, crc == 0, negative T, stride < 1: POLAR_E_ARG before the device is touched; T = 0 is POLAR_OK and
 * leaves stats alone). The trials run in chunks (512 MiB of LLR rows, or the "list_chunk_cw" knob); the counters are classified on
 * the device and read once, at the end of the call. */
#define POLAR_AD_MAX_STAGES 8
int polar_decode_scl_llr_adaptive_batch_dev(polar_code_t *h, const void *d_llr, int fmt, long B, const uint8_t *Ls, int n_s,
                                            uint8_t *d_out, double *d_pm, uint8_t *d_stage, uint8_t *d_crc_ok, void *stream);
int polar_decode_scl_llr_adaptive_batch(polar_code_t *h, const void *llr, int fmt, long B, const uint8_t *Ls, int n_s,
                                        uint8_t *out, double *pm, uint8_t *stage, uint8_t *crc_ok);
#define POLAR_AD_RUN 0      /* every trial */
#define POLAR_AD_ERR 1      /* delivered word differs from the sent info */
#define POLAR_AD_UNDET 2    /* ERR and crc_ok = 1 */
#define POLAR_AD_STAGE0 3   /* + s: trials delivered by stage s */
int polar_mc_batch_adaptive(polar_code_t *h, int constellation, uint64_t seed, uint64_t t0, long T, long stride,
                            const double *axis, int n_e, const uint8_t *Ls, int n_s, const uint8_t *enabled /*[n_e]*/,
                            uint64_t *stats /*[n_e][3 + n_s], ADDED to*/);

/* ---- SC-Flip: CRC-aided single-bit retries of SC decoding (Afisiadis, Balatsoukas-Stimming, Burg 2014) ----
 * (no member of the reference's class.) An SC pass with flip position c (c = -1: none) is plain successive cancellation in the LLR
 * domain with the reference's node arithmetic (PolarCode.cpp:437-451); leaf phi — a position in decoding order, the index space of
 * polar_get_frozen / polar_get_order — decides 0 if frozen, else 1 iff its LLR is negative, and at phi == c that decision is
 * inverted. There is no path metric. With T = max_flips in 0 .. POLAR_FLIP_MAX and T_eff = min(T, K + crc):
 *   pass 0   c = -1. Its unfrozen positions (info and check bits alike) ordered by |leaf LLR| ascending, equal magnitudes by position
 *            ascending, give cand[0 .. T_eff) and their magnitudes mag[]. If the word passes the handle's CRC — the check bits the CRC
 *            matrix gives for its K info bits equal its decided check bits — it is delivered: crc_ok = 1, n_dec = 1, flip = -1.
 *   retry t  (t = 0 .. T_eff-1) a whole pass with c = cand[t]; the first word that passes is delivered: crc_ok = 1, n_dec = t + 2,
 *            flip = cand[t].
 *   no pass  pass 0's word: crc_ok = 0, n_dec = T_eff + 1, flip = -1.
 *   out[B][K] uint8, crc_ok[B] uint8, n_dec[B] uint8, flip[B] int32, cand[B][max_flips] int32, mag[B][max_flips] double
 * cand / mag are pass 0's and are written for every row; entries t >= T_eff are -1 / +inf. out / d_out is required, the other five may
 * be NULL. Where the list-of-1 decode meets no tie between its two fork metrics, pass 0's word is polar_decode_scl_llr_batch_fmt(.., 1)
 * in mode 1; max_flips = 0 is that decode with a CRC verdict. One kernel, one codeword per wave with its whole state in LDS: n <= 12
 * (POLAR_E_UNSUPPORTED above, before the device is touched). polar_set_mode, polar_set_tuning and the latency threshold do not affect
 * it. POLAR_E_ARG, before the device is touched: NULL handle / rows / out, max_flips out of range, a handle with crc == 0, unknown fmt,
 * 16-bit rows at an odd address, negative B; B = 0 is POLAR_OK.
 *   _dev   device pointers, stream-ordered on `stream`, no host synchronisation: ONE launch (the retries loop in the kernel). Two calls
 *          on one handle and one stream need nothing between them. The first call of a handle uploads the kernel's schedule.
 *   host   host pointers: one copy of all B rows in, the launch, a wait, the copies out. A convenience form like the list call's.
 * polar_mc_batch_flip: like polar_mc_batch_adaptive: every ENABLED point of `axis` simulates all the trials {t0 + i*stride : i < T} and
 * ADDS to stats[ie*POLAR_FL_N + c] (host uint64). `constellation` as polar_mc_batch_list; POLAR_RX_MLC, NULL pointers, max_flips out of
 * range, crc == 0, negative T, stride < 1: POLAR_E_ARG before the device is touched; T = 0 is POLAR_OK and leaves stats alone. The
 * trials run in chunks (512 MiB of LLR rows, or the "list_chunk_cw" knob); the counters are read once, at the end of the call. */
#define POLAR_FLIP_MAX 64
int polar_decode_sc_flip_batch_dev(polar_code_t *h, const void *d_llr, int fmt, long B, int max_flips, uint8_t *d_out /*[B][K]*/,
                                   uint8_t *d_crc_ok /*[B]*/, uint8_t *d_n_dec /*[B]*/, int32_t *d_flip /*[B]*/,
                                   int32_t *d_cand /*[B][max_flips]*/, double *d_mag /*[B][max_flips]*/, void *stream);
int polar_decode_sc_flip_batch(polar_code_t *h, const void *llr, int fmt, long B, int max_flips, uint8_t *out, uint8_t *crc_ok,
                               uint8_t *n_dec, int32_t *flip, int32_t *cand, double *mag);
#define POLAR_FL_RUN 0      /* every trial */
#define POLAR_FL_ERR 1      /* delivered word differs from the sent info */
#define POLAR_FL_UNDET 2    /* ERR and crc_ok = 1 */
#define POLAR_FL_FIRST 3    /* crc_ok = 1 and n_dec == 1: pass 0 passed (with max_flips = 0 a failed word has n_dec = 1 too) */
#define POLAR_FL_FLIPPED 4  /* crc_ok = 1 and n_dec > 1: a retry delivered */
#define POLAR_FL_DECODES 5  /* sum of n_dec */
#define POLAR_FL_N 6
int polar_mc_batch_flip(polar_code_t *h, int constellation, uint64_t seed, uint64_t t0, long T, long stride, const double *axis,
                        int n_e, int max_flips, const uint8_t *enabled /*[n_e]*/, uint64_t *stats /*[n_e][POLAR_FL_N], ADDED to*/);

/* ---- SCAN: soft-output decoding by soft cancellation (Fayyaz, Barry 2014) ----
 * (no member of the reference's class.) The SC schedule with LLRs passed in both directions, `iters` (1 .. POLAR_SCAN_MAX_ITERS) times.
 * Layer 0 is the channel row, layer n the N leaves in decoding order — the index space of polar_get_frozen / polar_get_order; node v of
 * layer lam has N >> lam values and the children 2v (left) and 2v + 1 (right), which pair its neighbouring elements 2j, 2j + 1. Every
 * node carries L (towards the leaves; at layer 0 the caller's row) and B (towards the channel). A leaf's B is +inf if frozen, else 0;
 * every internal B is 0 before iteration 1. One iteration is one depth-first walk; at a node with values a, a0 = a[2j], a1 = a[2j+1]:
 *   L_left[j]  = f(a0, a1 + B_right[j])       (B_right: the previous iteration's)      ... the left child, which yields B_left ...
 *   L_right[j] = f(a0, B_left[j]) + a1                                                 ... the right child, which yields B_right ...
 *   B[2j]      = f(B_left[j], B_right[j] + a1),   B[2j+1] = f(B_left[j], a0) + B_right[j]
 * f is the f-node of decode_scl_llr (the reference's boxplus below 40, min-sum from 40 on; PolarCode.cpp:437-446) or, with
 * POLAR_SCAN_MINSUM, f(a, b) = sgn(a) sgn(b) min(|a|, |b|) with +0 where the min is 0. After the last iteration that ran:
 *   info_llr[B][K] double  info_llr[i] = the leaf L at order[i]
 *   out[B][K] uint8        out[i] = (info_llr[i] < 0): a zero of either sign decides 0
 *   ext[B][N] double       the B of layer 0: the extrinsic LLRs of the coded bits, indexed like the row (+inf where the frozen set alone
 *                          fixes a coded bit); the a-posteriori value is llr + ext
 *   crc_ok[B] uint8        the decided check bits at order[K .. K + crc) equal those the CRC matrix gives for out; 1 where crc == 0
 *   n_iter[B] uint8        the iterations that ran: `iters`, or with POLAR_SCAN_EARLY_STOP (crc > 0 only) the first whose decisions pass
 *                          the CRC — that iteration is the last
 * Rows must be finite. out / d_out is required, the other four may be NULL. One kernel, one codeword per wave with its whole state in
 * LDS: n <= 11 (POLAR_E_UNSUPPORTED above, before the device is touched). polar_set_mode and polar_set_tuning do not affect it.
 * POLAR_E_ARG, before the device is touched: NULL handle / rows / out, iters out of range, unknown flag bits, POLAR_SCAN_EARLY_STOP on a
 * handle with crc == 0, unknown fmt, 16-bit rows at an odd address, negative B; B = 0 is POLAR_OK.
 *   _dev   device pointers, stream-ordered on `stream`, no host synchronisation: ONE launch. Two calls on one handle and one stream
 *          need nothing between them. The first call of a handle uploads the kernel's schedule.
 *   host   host pointers: one copy of all B rows in, the launch, a wait, the copies out.
 * polar_mc_batch_scan: like polar_mc_batch_flip: every ENABLED point of `axis` simulates all the trials {t0 + i*stride : i < T} and ADDS
 * to stats[ie*POLAR_SN_N + c] (host uint64). `constellation` as polar_mc_batch_list; POLAR_RX_MLC, NULL pointers, iters or flags out of
 * range, negative T, stride < 1: POLAR_E_ARG before the device is touched; T = 0 is POLAR_OK and leaves stats alone. */
#define POLAR_SCAN_MINSUM 1
#define POLAR_SCAN_EARLY_STOP 2
#define POLAR_SCAN_MAX_ITERS 32
int polar_decode_scan_batch_dev(polar_code_t *h, const void *d_llr, int fmt, long B, int iters, int flags, uint8_t *d_out /*[B][K]*/,
                                double *d_info_llr /*[B][K]*/, double *d_ext /*[B][N]*/, uint8_t *d_crc_ok /*[B]*/,
                                uint8_t *d_n_iter /*[B]*/, void *stream);
int polar_decode_scan_batch(polar_code_t *h, const void *llr, int fmt, long B, int iters, int flags, uint8_t *out, double *info_llr,
                            double *ext, uint8_t *crc_ok, uint8_t *n_iter);
#define POLAR_SN_RUN 0      /* every trial */
#define POLAR_SN_ERR 1      /* decided word differs from the sent info */
#define POLAR_SN_UNDET 2    /* ERR on a code with a CRC, and crc_ok = 1 */
#define POLAR_SN_ITERS 3    /* sum of n_iter */
#define POLAR_SN_N 4
int polar_mc_batch_scan(polar_code_t *h, int constellation, uint64_t seed, uint64_t t0, long T, long stride, const double *axis,
                        int n_e, int iters, int flags, const uint8_t *enabled /*[n_e]*/, uint64_t *stats /*[n_e][POLAR_SN_N], ADDED to*/);

/* ---- systematic polar coding (Arikan 2011) ----
 * (no member of the reference's class.) The message bits appear verbatim in the codeword; codebook, decoders and BLER are those of the
 * plain code, the message BER is about half. Notation: K' = K + crc, A' = order[0 .. K'), mask = its indicator, z = butterfly(u) (the
 * encoder's stages u[a] ^= u[a + inc] in natural order), coded[i] = z[bitrev(i)], H the CRC matrix, T x = mask & butterfly(x),
 * syndrome(u)[r] = (sum_j H[r][j] u[order[j]]) ^ u[order[K + r]].
 *   T^-1     u = x, then `depth` times u = x ^ u ^ T u; depth = the least t >= 1 after which every unit vector of A' is solved
 *            (1 for every constructed code; at most n).
 *   parity   the CRC stays a constraint on u, where every decoder checks it, so crc of the K' unfrozen positions of z are not free:
 *            walking i = K' - 1 .. 0 with p = order[i], D_p = T^-1 e_p and c_p = syndrome(D_p), p is accepted when c_p is linearly
 *            independent over GF(2) of the accepted columns, until crc are. par_u = the accepted positions in that order, msg_u = A'
 *            without them in the order of `order`, Q = the accepted columns, n_swapped = the accepted positions outside order[K .. K').
 *   precode  m[K] -> u_info[K]: x0[msg_u[i]] = m[i]; u = T^-1 x0; zP = Q^-1 syndrome(u); u ^= sum_r zP[r] D_{par_u[r]};
 *            u_info[i] = u[order[i]]. The systematic codeword is polar_encode(u_info), and coded[bitrev(msg_u[i])] = m[i].
 *   message  u_info[K] -> m[K]: m[i] = butterfly(u with u[order[i]] = u_info[i], check bits recomputed)[msg_u[i]] — polar_encode
 *            followed by a gather, valid for ANY u_info (a decoder's output); m differs from the sent message exactly when u_info
 *            differs from the sent one.
 * polar_get_sys_info / polar_get_sys_positions: depth, n_swapped, and the coded-row indices pos[i] = bitrev(msg_u[i]) [K],
 * par[r] = bitrev(par_u[r]) [crc] (any output may be NULL). Host tables only: no device is needed. The tables are built at the
 * first systematic call of a handle and again after polar_set_crc_matrix.
 * polar_encode_sys_batch[_dev]: msg [B][K] -> coded [B][N] and / or u_info [B][K] (either may be NULL, not both).
 * polar_sys_message_batch[_dev]: u_info [R][K] -> msg [R][K], R any row count (the cand [B][L][K] of a list call are B L rows);
 * msg == u_info (in place) is allowed.
 * polar_sys_soft_batch[_dev]: soft message outputs from a soft-output decode: msg_llr[b][i] = widen(llr[b][pos[i]]) + ext[b][pos[i]]
 * (llr [B][N] of `fmt`, ext [B][N] doubles, e.g. polar_decode_scan_batch_dev's; one fp64 addition, +inf passes through).
 * polar_synth_sys_llr_dev: polar_synth_llr_dev (constellation 0 or POLAR_CONST_BPSK, s_or_snr = polar_snr_sqrt_linear(h, Eb/N0)) or
 * polar_synth_bicm_llr_dev (POLAR_CONST_ASK*, s_or_snr = the SNR in dB) with the systematic codeword: trial t sends as MESSAGE the
 * info bits those calls draw for trial t, over the same noise. d_llr [B][N] is required; d_msg [B][K] (the message) and d_u_info
 * [B][K] (its precoded word, what a decoder's output is compared with) may be NULL.
 * polar_mc_batch_sys: like polar_mc_batch_list: every ENABLED (L, point) simulates all the trials {t0 + i*stride : i < T} of the
 * systematic workload with decode_scl_llr at that list size and ADDS to stats[(li*n_e + ie)*POLAR_SY_N + c] (host uint64), counted on
 * the same decodes.
 * All kernels are bit-packed (a codeword is N / 64 words in the lanes of a wave; no LDS); the _dev forms are stream-ordered with no
 * host synchronisation, one launch each (polar_synth_sys_llr_dev: three), and two calls on one handle and one stream need nothing
 * between them; the first systematic call of a handle uploads the tables. Host forms: copies in, the launch, a wait, the copies out.
 * POLAR_E_ARG before the device is touched: NULL handle or required pointer, unknown fmt, 16-bit rows at an odd address, unknown
 * constellation or POLAR_RX_MLC, a list size out of range, negative B / R / T, stride < 1; B = 0 (R = 0, T = 0) is POLAR_OK and
 * writes nothing. */
int polar_get_sys_info(polar_code_t *h, int *depth, int *n_swapped);
int polar_get_sys_positions(polar_code_t *h, uint16_t *pos /*[K]*/, uint16_t *par /*[crc]*/);
int polar_encode_sys_batch(polar_code_t *h, const uint8_t *msg /*[B][K]*/, long B, uint8_t *coded /*[B][N] or NULL*/,
                           uint8_t *u_info /*[B][K] or NULL*/);
int polar_encode_sys_batch_dev(polar_code_t *h, const uint8_t *d_msg, long B, uint8_t *d_coded, uint8_t *d_u_info, void *stream);
int polar_sys_message_batch(polar_code_t *h, const uint8_t *u_info /*[R][K]*/, long R, uint8_t *msg /*[R][K]*/);
int polar_sys_message_batch_dev(polar_code_t *h, const uint8_t *d_u_info, long R, uint8_t *d_msg, void *stream);
int polar_sys_soft_batch(polar_code_t *h, const void *llr, int fmt, const double *ext, long B, double *msg_llr /*[B][K]*/);
int polar_sys_soft_batch_dev(polar_code_t *h, const void *d_llr, int fmt, const double *d_ext, long B, double *d_msg_llr, void *stream);
int polar_synth_sys_llr_dev(polar_code_t *h, int constellation, uint64_t seed, uint64_t trial0, long B, double s_or_snr,
                            double *d_llr, uint8_t *d_msg, uint8_t *d_u_info, void *stream);
#define POLAR_SY_RUN 0      /* every trial */
#define POLAR_SY_ERR 1      /* decoded u-domain word differs from the sent one (equally: the recovered message does) */
#define POLAR_SY_BIT_MSG 2  /* wrong message bits */
#define POLAR_SY_BIT_U 3    /* wrong u-domain info bits, on the same decodes */
#define POLAR_SY_N 4
int polar_mc_batch_sys(polar_code_t *h, int constellation, uint64_t seed, uint64_t t0, long T, long stride, const double *axis,
                       int n_e, const uint8_t *L, int n_L, const uint8_t *enabled /*[n_L*n_e]*/,
                       uint64_t *stats /*[n_L*n_e][POLAR_SY_N], ADDED to*/);

/* ---- rate matching: puncturing, shortening, repetition ----
 * (no member of the reference's class.) E coded bits are sent instead of the N = 2^n of the mother code. Conventions: z = butterfly(u)
 * in natural order, coded[i] = z[bitrev(i)], an LLR > 0 means bit 0.
 *   pattern  sel uint16 [E], 1 <= E <= 8 N: transmit position e carries coded[sel[e]]; known uint8 [N]: coded positions that are not
 *            sent and are 0 in every codeword (shortened). A coded position in neither is punctured; a position that occurs several
 *            times in sel is repeated.
 *   schemes  polar_rm_pattern(n, E, scheme, Kp, sel, known) (host only, no handle; known is zero-filled first and may be NULL for
 *            the schemes that set none; Kp = K + crc is read by POLAR_RM_NR alone):
 *              POLAR_RM_PUNCTURE (E < N)  sel[e] = N - E + e;
 *              POLAR_RM_SHORTEN  (E < N)  sel[e] = e, known[E .. N) = 1;
 *              POLAR_RM_REPEAT   (E >= N) sel[e] = e mod N;
 *              POLAR_RM_NR       (n >= 5) the sub-block interleaver and bit selection of 3GPP TS 38.212 §5.4.1 applied to z (NR's d):
 *                                P32 = 0 1 2 4 3 5 6 7 8 16 9 17 10 18 11 19 12 20 13 21 14 22 15 23 24 25 26 28 27 29 30 31,
 *                                J(j) = P32[floor(32 j / N)] (N / 32) + j mod (N / 32), y[j] = bitrev(J(j)) as a coded-row index;
 *                                E >= N: sel[e] = y[e mod N]; else Kp / E <= 7 / 16: sel[e] = y[e + N - E] (puncture); else
 *                                sel[e] = y[e], known[y[E .. N)] = 1 (shorten). The pattern only: NR's extra pre-freezing and its
 *                                reliability sequence are not part of it.
 *   forced   polar_rm_forced(n, sel, E, known, forced) (host only): the leaves a design for this pattern must freeze, as a mask
 *            forced uint8 [N] by leaf index; their number is returned (negative: an error code): for every known coded position p every leaf b with
 *            b & bitrev(p) == bitrev(p) (z is 0 there for every word exactly when all of them are frozen), and the zero-capacity
 *            leaves of the punctured set: a boolean row in coded order, true at the punctured positions, through n stages of
 *            [c1 | c2, c1 & c2] (c1 / c2 = the even / odd entries, the layout of calculate_awgn_polarization.m), then bit reversal.
 *   recover  rx [B][E] of any POLAR_LLR_* format -> llr fp64 [B][N]: at a known position short_llr (a handle setting, finite, > 0,
 *            1000.0 by convention); at every other position acc = +0.0, then acc = acc + widen(rx[b][e]) over the e with sel[e] = p in
 *            ascending e — plain fp64 additions, no contraction, no reordering; a punctured position is +0.0. Bit patterns are the
 *            contract.
 * polar_set_rate_match(h, sel, E, known or NULL, short_llr): the pattern of the handle; E = 0 clears it. POLAR_E_ARG, with a message
 * naming the first offender: E outside [1, 8 N], sel[e] >= N, a known position that is also sent, a leaf b >= bitrev(p) bitwise of a
 * known position p that is unfrozen in this handle (the word would not be 0 there), short_llr not finite or not positive. A punctured
 * pattern whose zero-capacity leaves are unfrozen is accepted: the caller's loss, not an inconsistency.
 * polar_get_rate_match: E (0: none set), and where E > 0 sel [E], known [N], short_llr (any output may be NULL).
 * polar_rate_match_batch[_dev]: coded uint8 [B][N] -> tx uint8 [B][E]. polar_rate_recover_batch[_dev]: rx [B][E] of fmt -> llr [B][N].
 * polar_decode_scl_llr_rm_batch[_dev]: recover into the handle's scratch, then decode_scl_llr at list size L (out [B][K], d_pm [B] or
 * NULL). A pattern with any punctured or known position decodes in the LLR-domain kernel family for that call (as polar_set_mode(h, 1)
 * would, for this call only): the fast kernels would hand every such row to their fallback pass. A pure repetition pattern takes
 * the handle's own choice.
 * polar_snr_sqrt_linear_rm: polar_snr_sqrt_linear with E in place of N (NaN without a pattern).
 * polar_synth_rm_llr_dev: the rate-matched workload: trial t = trial0 + b draws the info bits polar_synth_llr_dev draws for trial t,
 * encodes them, and rx[b][e] = polar_synth_llr(s, coded[sel[e]], z_e), z_e = element e & 1 of polar_synth_noise_pair(seed, t, e >> 1)
 * (include/polar_synth.h); d_rx fp64 [B][E], d_info [B][K] or NULL.
 * polar_mc_batch_rm: like polar_mc_batch_list on the Eb/N0 axis (BPSK): every ENABLED (L, point) simulates the trials
 * {t0 + i*stride : i < T} of that workload at s = polar_snr_sqrt_linear_rm(h, ebno), decodes them as polar_decode_scl_llr_rm_batch_dev
 * does and ADDS to stats[(li*n_e + ie)*POLAR_RM_N + c].
 * The _dev forms are stream-ordered with no host synchronisation, and two calls on one handle and one stream need nothing between
 * them; the first call after polar_set_rate_match uploads the tables. Host forms: copies in, the launches, a wait, the copies out.
 * POLAR_E_ARG before the device is touched: no pattern set, NULL handle or required pointer, unknown fmt, 16-bit rows at an odd
 * address, a list size out of range, negative B / T, stride < 1; B = 0 (T = 0) is POLAR_OK and writes nothing.
 * polar_ga_construction_init: the Gaussian-approximation design started from a per-position vector: init [n_points][N] in coded
 * order takes the place of the mean LLR of polar_ga_construction (one block of N), then the same polarization, bit reversal, stable
 * descending sort and prefix sums; the leaves with forced[leaf] != 0 (uint8 [N]; NULL: none) are moved to the END of every `order` row
 * in ascending index, whatever their value (the phi tables are not exact at 0). bler_prefix follows the order that is returned. */
#define POLAR_RM_PUNCTURE 0
#define POLAR_RM_SHORTEN 1
#define POLAR_RM_REPEAT 2
#define POLAR_RM_NR 3
int polar_rm_pattern(int n, int E, int scheme, int Kp, uint16_t *sel /*[E]*/, uint8_t *known /*[N]*/);
int polar_rm_forced(int n, const uint16_t *sel, int E, const uint8_t *known /*[N] or NULL*/, uint8_t *forced /*[N], by leaf index*/);
int polar_set_rate_match(polar_code_t *h, const uint16_t *sel, int E, const uint8_t *known /*[N] or NULL*/, double short_llr);
int polar_get_rate_match(const polar_code_t *h, int *E, uint16_t *sel, uint8_t *known, double *short_llr);
int polar_rate_match_batch(polar_code_t *h, const uint8_t *coded /*[B][N]*/, long B, uint8_t *tx /*[B][E]*/);
int polar_rate_match_batch_dev(polar_code_t *h, const uint8_t *d_coded, long B, uint8_t *d_tx, void *stream);
int polar_rate_recover_batch(polar_code_t *h, const void *rx /*[B][E] of fmt*/, int fmt, long B, double *llr /*[B][N]*/);
int polar_rate_recover_batch_dev(polar_code_t *h, const void *d_rx, int fmt, long B, double *d_llr, void *stream);
int polar_decode_scl_llr_rm_batch(polar_code_t *h, const void *rx, int fmt, long B, int L, uint8_t *out /*[B][K]*/);
int polar_decode_scl_llr_rm_batch_dev(polar_code_t *h, const void *d_rx, int fmt, long B, int L, uint8_t *d_out, double *d_pm,
                                      void *stream);
double polar_snr_sqrt_linear_rm(const polar_code_t *h, double ebno_db);
int polar_synth_rm_llr_dev(polar_code_t *h, uint64_t seed, uint64_t trial0, long B, double s, double *d_rx, uint8_t *d_info,
                           void *stream);
#define POLAR_RM_RUN 0      /* every trial */
#define POLAR_RM_ERR 1      /* decoded info bits differ from the sent ones */
#define POLAR_RM_BIT 2      /* wrong info bits */
#define POLAR_RM_N 3
int polar_mc_batch_rm(polar_code_t *h, uint64_t seed, uint64_t t0, long T, long stride, const double *ebno, int n_e, const uint8_t *L,
                      int n_L, const uint8_t *enabled /*[n_L*n_e]*/, uint64_t *stats /*[n_L*n_e][POLAR_RM_N], ADDED to*/);
int polar_ga_construction_init(int n, const double *init /*[n_points][N], coded order*/, const uint8_t *forced /*[N] by leaf index, or NULL*/,
                               int n_points, double phi_dx, double *channels, uint16_t *order, double *bler_prefix);

/* ---- PolarCode::decode_scl_p1(PolarCode.cpp:110-128; PolarCode.m:299-310) ---- */
int polar_decode_scl_p1(polar_code_t *h, const double *p1 /*[N]*/, const double *p0 /*[N]*/, int L, uint8_t *out /*[K]*/);
int polar_decode_scl_p1_batch(polar_code_t *h, const double *p1, const double *p0, long B, int L, uint8_t *out);

/* ---- PolarM decode_sc_p1 (PolarCode.m:290-295, 870-895): SC on p1 = P(bit = 1) ----
 * out are doubles, as MATLAB returns them: 0 / 1, 0.5 where a leaf probability is exactly 0.5
 * (sign(0) = 0 at PolarCode.m:873), and NaN where a leaf probability is NaN (sign(NaN) = NaN: vnop,
 * PolarCode.m:893-895, divides 0 by 0 when its inputs contradict each other with certainty, e.g. p1 = 0, 1
 * on a pair whose first bit is frozen; once a decision is NaN the partial sums carry it to later leaves). */
int polar_decode_sc_p1(polar_code_t *h, const double *p1 /*[N]*/, double *out /*[K]*/);
int polar_decode_sc_p1_batch(polar_code_t *h, const double *p1, long B, double *out);

/* ---- synthetic BPSK/AWGN workload (include/polar_synth.h), generated on the device ----
 * trials [trial0, trial0+B): info bits (block = trial/100), encode, BPSK, AWGN, LLR with
 * the arithmetic of PolarCode.cpp:715,744-752; `s` = polar_snr_sqrt_linear(h, EbN0_dB).
 * d_info (optional) receives the transmitted info bits [B*K]. */
double polar_snr_sqrt_linear(const polar_code_t *h, double ebno_db);   /* PolarCode.cpp:744-745 */
int polar_synth_llr_dev(polar_code_t *h, uint64_t seed, uint64_t trial0, long B, double s,
                        double *d_llr, uint8_t *d_info, void *stream);
/* compare decoded vs sent info bits on the device: *d_err_count += #codewords that differ */
int polar_count_errors_dev(polar_code_t *h, const uint8_t *d_a, const uint8_t *d_b, long B,
                           unsigned long long *d_err_count, void *stream);

/* ---- PolarCode::get_bler_quick (PolarCode.cpp:658-785; PolarCode.m:781-850) ----
 * Batched Monte-Carlo on the synthetic workload. Semantics of the reference kept per trial
 * (one noise vector shared by every (L, Eb/N0); ascending Eb/N0 with "decoded at a lower
 * Eb/N0 => counted, not simulated", :728-742); the early stop `num_err > max_err` (:725)
 * is evaluated between rounds of `batch` trials (batch = 1 reproduces the reference's per-run granularity).
 * batch = 0 (the default of the host mirrors) picks the rounds itself: max(256, 2 max_err) trials first, then every
 * round as large as all rounds before it together (at most 262144) — a point overshoots the reference's stopping
 * time by less than 2x, and long sweeps still reach full-size launches. Reference defaults: max_runs = 1000,
 * max_err = 100 (:661-662); PolarM: 500 / 50 (PolarCode.m:788-789).
 * A round runs stream-ordered on the device (alive lists compacted there, PolarCode.cpp:728-742); the host reads
 * the 2 n_L n_e counters once per round. */
int polar_get_bler_quick(polar_code_t *h, const double *ebno, int n_e, const uint8_t *L, int n_L,
                         long max_runs, long max_err, uint64_t seed, long batch,
                         double *bler_out /*[n_L*n_e]*/);
/* PolarM's second output (PolarCode.m:781, 839, 848): ber[i] = (differing info bits of the block errors) / num_run,
 * per run as the reference computes it (NOT divided by K). Layout [n_L][n_e] like bler. */
int polar_get_bler_quick_ber(polar_code_t *h, const double *ebno, int n_e, const uint8_t *L, int n_L,
                             long max_runs, long max_err, uint64_t seed, long batch,
                             double *bler_out /*[n_L*n_e]*/, double *ber_out /*[n_L*n_e]*/);
/* The same sweep sharded over `n_dev` GPUs of this node from ONE host process (the C++ / MATLAB hosts): device
 * devices[d] (NULL = 0..n_dev-1) simulates the trials d, d + n_dev, ... of every round on its own stream, with its
 * own copy of the code tables and scratch (owned by `h`); the round's counters are summed with one RCCL
 * ncclAllReduce(uint64, sum) over xGMI (bound at run time; a host-side sum when RCCL cannot be loaded, or with
 * POLAR_NO_RCCL set when the handle was created). Counter-based inputs make the counters independent of n_dev for a given
 * `batch` (the automatic rounds grow with the device count: 262144 trials per device). *used_rccl (optional) reports
 * which path summed the counters. ber_out may be NULL. A device may be listed once (the test build of the library has a hook
 * that lifts this so that one GPU can stand in for several: include/polar_amd_debug.h). One worker thread per device lives on
 * the handle between calls (created with the communicators). */
int polar_get_bler_quick_multi(polar_code_t *h, const int *devices, int n_dev, const double *ebno, int n_e,
                               const uint8_t *L, int n_L, long max_runs, long max_err, uint64_t seed, long batch,
                               double *bler_out, double *ber_out, int *used_rccl);

/* General form of the sweep: `constellation` 0 / POLAR_CONST_BPSK = BPSK over AWGN with the Eb/N0 axis of
 * PolarCode.cpp:744-753 (what the three entry points above simulate); POLAR_CONST_ASK{4,8,16}_{GRAY,SP} (include/polar_synth.h) =
 * the ASK Gray + BICM front end of PolarM/Constellation.m with the SNR axis and fresh info bits every run
 * (PolarM/main_MC_CC_Comparison.m:44-119: BASELINE configuration 5, sharded over the GPUs of the node from one host
 * process). devices == NULL: 0..n_dev-1 (with n_dev == 1: the handle's own device). Optional outputs (may be NULL):
 * ber_out, the raw counters err_out / run_out [n_L*n_e] (block errors and simulated-or-counted runs per point: what the
 * estimates are made of, and what two runs are compared by), *rounds_out = rounds the call took, *used_rccl.
 * Rounds: `batch` trials over all devices, or (batch == 0) geometric up to 262144 trials PER DEVICE.
 * The rounds are pipelined on the device — a step decodes point 1 of the newest round together with the later points of the
 * rounds before it, one launch per list size — with exactly the counters, early stop and run counts of the round-after-round
 * loop; the counters are reduced once per step.
 * Failure handling: a device that fails before the step's collective keeps every device out of it; a device whose
 * collective enqueue fails makes every device abort its communicator before it waits; a step that exceeds the watchdog
 * (1800 s; include/polar_amd_debug.h "multi_timeout_s") is ended in three bounded stages ("multi_grace_s", 10 s each): the workers are
 * signalled and abort their own communicators, what is left is aborted from the calling thread, and a worker that still does
 * not answer is given up — the call returns, the handle accepts no further get_bler_quick* calls and polar_destroy frees
 * nothing of it. Otherwise the call returns POLAR_E_DEVICE and the next call rebuilds the communicators. */
int polar_get_bler_quick_multi_ex(polar_code_t *h, int constellation, const int *devices, int n_dev, const double *axis, int n_e,
                                  const uint8_t *L, int n_L, long max_runs, long max_err, uint64_t seed, long batch,
                                  double *bler_out, double *ber_out, uint64_t *err_out, uint64_t *run_out, long *rounds_out,
                                  int *used_rccl);

/* The same sweep with the trials shared by `world` PROCESSES (one per GPU, as a process-group or MPI launcher starts them): this process is
 * `rank`, its handle's device simulates the trials rank, rank + world, ... of every round, and after every step `reduce` is
 * called — collectively, on every rank, the same number of times — to SUM the n uint64 counters in place over the ranks
 * (e.g. an all-reduce of the process group; return non-zero to fail the call). A rank whose own step failed (launch error,
 * watchdog) still makes this call once, with a failure flag in the last counter: every rank then returns POLAR_E_DEVICE from
 * the same step and none is left waiting in the collective. Counters, estimates and rounds are those of
 * polar_get_bler_quick_multi_ex with world devices. polar_amd/montecarlo.py drives it with its process group's all-reduce. */
typedef int (*polar_reduce_fn)(void *user, uint64_t *counters, int n);
int polar_get_bler_quick_rank(polar_code_t *h, int constellation, int rank, int world, polar_reduce_fn reduce, void *user,
                              const double *axis, int n_e, const uint8_t *L, int n_L, long max_runs, long max_err, uint64_t seed,
                              long batch, double *bler_out, double *ber_out, uint64_t *err_out, uint64_t *run_out, long *rounds_out);

/* step-wise Monte-Carlo for multi-GPU drivers: simulate trials {t0 + i*stride : i < T} for
 * every enabled (L, Eb/N0) point and ADD to err/run (host uint64 [n_L*n_e]). */
int polar_mc_batch(polar_code_t *h, uint64_t seed, uint64_t t0, long T, long stride,
                   const double *ebno, int n_e, const uint8_t *L, int n_L,
                   const uint8_t *enabled /*[n_L*n_e]*/, uint64_t *err, uint64_t *run);
/* same, also accumulating the differing info bits of the block errors (PolarM's num_bit_err, PolarCode.m:840) */
int polar_mc_batch_ber(polar_code_t *h, uint64_t seed, uint64_t t0, long T, long stride,
                       const double *ebno, int n_e, const uint8_t *L, int n_L,
                       const uint8_t *enabled /*[n_L*n_e]*/, uint64_t *err, uint64_t *bit_err, uint64_t *run);

/* ---- ASK Gray + BICM front end (PolarM/Constellation.m:84-93, 123-144; sweep conventions of
 * PolarM/main_MC_CC_Comparison.m:88-96) for the 16-ASK configuration: `constellation` is
 * POLAR_CONST_ASK{4,8,16}_{GRAY,SP} (include/polar_synth.h), the sweep axis is the SNR in dB
 * (Eb/N0 = snr_db + 10log10(N/K) - 10log10(n_bits), main_MC_CC_Comparison.m:121), info bits are
 * fresh every run. Same counters/semantics as polar_mc_batch. */
int polar_synth_bicm_llr_dev(polar_code_t *h, int constellation, uint64_t seed, uint64_t trial0, long B,
                             double snr_db, double *d_llr, uint8_t *d_info, void *stream);
int polar_mc_batch_bicm(polar_code_t *h, int constellation, uint64_t seed, uint64_t t0, long T, long stride,
                        const double *snr_db, int n_s, const uint8_t *L, int n_L,
                        const uint8_t *enabled, uint64_t *err, uint64_t *run);

/* ---- the Constellation class beside PolarCode (PolarM/Constellation.m) and the symbol-domain BICM receiver ----
 * `constellation` is a POLAR_CONST_* id 1 .. 7 (include/polar_synth.h: BPSK, 4- / 8- / 16-ASK with Gray or set-partition labels),
 * nb its bits per symbol, M = floor(N / nb) symbols per row of N coded bits.
 *   polar_modulate        Constellation.modulate (:84-93, symbol index = sum 2^j bit_j, LSB first) on the host: coded [B][N]
 *                         -> normalised points sym [B][M]; the N - M*nb tail bits of a row are not sent. No handle, no device.
 *   polar_demap_bicm      Constellation.compute_llr_bicm (:123-144) on the device: y [B][M] with noise variance n0 -> llr [B][N]
 *                         and / or p1 [B][N] (either may be NULL, not both), position i*nb + j = label bit j of symbol i, the
 *                         tail positions M*nb .. N-1 llr = 0, p1 = 0.5 (main_MC_CC_Comparison.m:94). Every value is bit for bit
 *                         polar_synth_bicm_demap2 of include/polar_synth.h (fixed-order exp / log, the same on host and device).
 *                         Host pointers, no handle; _dev: device pointers, asynchronous on `stream`; _f32: single-precision
 *                         symbols, each widened exactly.
 *   polar_decode_bicm_batch   decode_scl_llr from received symbols: the result is bit for bit polar_decode_scl_llr_batch on
 *                         polar_demap_bicm's LLRs of the same y (for _f32: of (double)y[i]), from 1 / nb (double) or 1 / 2nb
 *                         (float) of the input bytes. Host pointers: the staging, pipelining and latency paths of
 *                         polar_decode_scl_llr_batch, chosen for a given B as that function chooses them, with the symbols
 *                         demapped on the device in front of the decode. _dev: device pointers, stream-ordered, no host
 *                         synchronisation (the handle's LLR buffer is grown on demand like its other scratch); d_pm as
 *                         polar_decode_scl_llr_batch_dev.
 *   polar_synth_bicm_sym_dev  the received symbols [B][M] of the trials for which polar_synth_bicm_llr_dev gives the LLRs.
 * POLAR_E_ARG: NULL pointers, constellation 0 or unknown, n0 not finite or <= 0, L out of range, negative B, N outside
 * [1, 2^POLAR_MAX_N_LOG2]; B = 0 is POLAR_OK. */
int polar_modulate(int constellation, const uint8_t *coded, int N, long B, double *sym);
int polar_demap_bicm(int constellation, const double *y, int N, long B, double n0, double *llr, double *p1);
int polar_demap_bicm_f32(int constellation, const float *y, int N, long B, double n0, double *llr, double *p1);
int polar_demap_bicm_dev(int constellation, const double *d_y, int N, long B, double n0, double *d_llr, double *d_p1, void *stream);
int polar_demap_bicm_dev_f32(int constellation, const float *d_y, int N, long B, double n0, double *d_llr, double *d_p1, void *stream);
int polar_decode_bicm_batch(polar_code_t *h, int constellation, const double *y, double n0, long B, int L, uint8_t *out);
int polar_decode_bicm_batch_f32(polar_code_t *h, int constellation, const float *y, double n0, long B, int L, uint8_t *out);
int polar_decode_bicm_batch_dev(polar_code_t *h, int constellation, const double *d_y, double n0, long B, int L, uint8_t *d_out,
                                double *d_pm, void *stream);
int polar_decode_bicm_batch_dev_f32(polar_code_t *h, int constellation, const float *d_y, double n0, long B, int L, uint8_t *d_out,
                                    double *d_pm, void *stream);
int polar_synth_bicm_sym_dev(polar_code_t *h, int constellation, uint64_t seed, uint64_t trial0, long B, double snr_db,
                             double *d_y, uint8_t *d_info, void *stream);

/* ---- Monte-Carlo code construction (PolarM/PolarCode.m:143-196 `monte_carlo`, receiver 'bicm',
 * with the genie-aided SC decoder `polar_decode_monte` :897-914). No handle: the result is what a
 * code is built FROM. For runs trial0 .. trial0+num_runs-1 (counter-based inputs, polar_synth.h):
 * N random message bits, polar transform, `constellation` (POLAR_CONST_BPSK or _ASK{4,8,16}_{GRAY,SP})
 * at the design SNR (sigma = sqrt(1/2) * 10^(-snr/20), n0 = sigma^2, :170), BICM p1, genie SC;
 * num_err[i] (host uint64 [2^n]) is INCREMENTED by the number of runs whose position i decided
 * wrongly — the table the reference writes to CodeConstructionData/MC_block_length_*.txt (:120-124)
 * and turns into a frozen set by a stable ascending sort (:126-135; polar_create_explicit /
 * PolarCode.from_counts). `batch` = runs per launch (0 = default). Disjoint trial ranges may be
 * summed across GPUs. */
int polar_mc_construction(int n, int constellation, double design_snr_db, uint64_t seed, uint64_t trial0,
                          long num_runs, long batch, uint64_t *num_err);

/* ---- multi-level coding (MLC) receiver (PolarM/main_MC_CC_Comparison.m:55-62, 98-110; PolarCode.m:155-161, 180-190) ----
 * POLAR_RX_MLC OR-ed into the `constellation` argument of polar_get_bler_quick_multi_ex, polar_get_bler_quick_rank and
 * polar_mc_construction selects the MLC receiver instead of BICM: nb = n_bits of the constellation component polar codes of
 * length M = N / nb (message positions layer-major: component k owns positions k*M .. (k+1)*M - 1; the handle's frozen set
 * is sliced the same way), component k carried by label bit k of the symbols, multistage SC decoding in the probability
 * domain with each layer demapped conditioned on the re-encoded decisions of the layers below (Constellation.m:95-121).
 * Construction: genie-aided per layer, counts layer-major. Sweep axis: SNR in dB, fresh info every run, list size 1 only.
 * Workload definition: include/polar_synth.h. Refused with POLAR_E_ARG: a handle with crc_size > 0, a list size other than 1,
 * an unknown constellation, N / nb not a power of two >= 2 (8-ASK at N = 1024).
 * The entry points below take the constellation with or without the flag:
 *   polar_encode_mlc      info [B][K] (host) -> coded [B][N] (host) in modulation order (symbol i, label bit k at i*nb + k);
 *   polar_decode_mlc      received symbols y [B][M] (host), noise variance n0 -> decisions [B][K] as doubles (decode_sc_p1
 *                         convention: 0.5 or NaN where a leaf is undecided), host pointers;
 *   polar_decode_mlc_dev  the same on device pointers, stream-ordered on `stream`;
 *   polar_synth_mlc_dev   the sweep's trials trial0 .. trial0+B-1 at `snr_db`: symbols [B][M] and sent info [B][K] (may be NULL). */
#define POLAR_RX_MLC 0x100
int polar_encode_mlc(polar_code_t *h, int constellation, const uint8_t *info, long B, uint8_t *coded);
int polar_decode_mlc(polar_code_t *h, int constellation, const double *y, double n0, long B, double *out);
int polar_decode_mlc_dev(polar_code_t *h, int constellation, const double *d_y, double n0, long B, double *d_out, void *stream);
int polar_synth_mlc_dev(polar_code_t *h, int constellation, uint64_t seed, uint64_t trial0, long B, double snr_db,
                        double *d_y, uint8_t *d_info, void *stream);

/* ---- Gaussian-approximation (GA) code construction (PolarM/PolarCode.m:198-255 `ga_code_construction`,
 * GaussianApproximation/, CapacityHelper/, main_GA_CC_Comparison.m). No handle, like polar_mc_construction. fp64 on the
 * device; grids and index rules in DESIGN.md §8b. Supported constellations: POLAR_CONST_BPSK, _ASK4_{GRAY,SP},
 * _ASK16_{GRAY,SP}; 8-ASK (the reference splits N into thirds), N / n_bits below 2 and unknown ids give POLAR_E_ARG.
 * sigma = sqrt(1/2) * 10^(-snr/20), n0 = sigma^2 (Constellation.m:251).
 *   polar_bicm_capacity   get_bicm_capacity (Constellation.m:250-286): out[n][nb], integral over y_k = -ymax + k*dy,
 *                         ymax = max(points) + 6 sigma + 1, dy = 0.1 sigma, P = floor(2 ymax / dy + 1e-9) + 1 points;
 *   polar_mlc_capacity    get_mlc_capacity (:190-248): the same per layer, conditioned on the lower label bits, dy = 0.01 sigma;
 *   polar_bpsk_capacity   get_bpsk_cap.m: out[n] (n0 = 10^(-snr/10) / 2, dy = 0.001 sqrt(n0), ymax = min(1e4, 4 + 3 sqrt(n0)));
 *   polar_ga_phi_tables   initialize_phi.m at x step phi_dx: fwd[10002] (x = k * 0.01) and inv[100001] (largest x = k * phi_dx
 *                         whose -log(phi) falls in bin ceil(-log(phi) / 1e-3), 0 where none does);
 *   polar_polarized_counts  get_polarized_capacity (:288-370) for symbols trial0 .. trial0+num_sym-1 (the Monte-Carlo
 *                         construction's runs at N = nb, include/polar_synth.h): u-LLR histograms counts[n][nb][801][2]
 *                         (bin floor((clip(u, +-100) + 100) / 0.25), NaN -> bin 0; sent bit) are INCREMENTED, so disjoint
 *                         seed or symbol ranges add up;
 *   polar_polarized_capacity_from_counts  the entropy difference of those histograms, min(cap, 1) -> out[n][nb];
 *   polar_polarized_capacity  both, for symbols 0 .. num_sym-1;
 *   polar_ga_mean_llr     get_bpsk_llr_for_capacity.m: 4 * 10^(s_k / 10) for the first s_k = -20 + k * 0.01 whose BPSK capacity
 *                         (polar_bpsk_capacity) reaches the value, s_4000 = 20 dB when none does;
 *   polar_ga_construction the design points snr_db[n_points] of `constellation` (| POLAR_RX_MLC for the MLC receiver): the
 *                         capacities (given in capacity[n_points][nb], or NULL: the integral for BPSK and MLC, the polarized
 *                         capacity of 250 000 symbols of `seed` for multi-bit BICM), the mean LLRs, calculate_awgn_polarization
 *                         per sub-block of N / nb with the phi tables of phi_dx, bit reversal -> channels[n_points][N]; the
 *                         stable descending order of the channels -> order[n_points][N] (most reliable first); prefix sums
 *                         of qfunc(sqrt(c) / sqrt(2)) along it -> bler_prefix[n_points][N] (entry K-1: the BLER estimate of
 *                         K unfrozen positions). Any of the three outputs may be NULL. */
int polar_bicm_capacity(int constellation, const double *snr_db, int n, double *out);
int polar_mlc_capacity(int constellation, const double *snr_db, int n, double *out);
int polar_bpsk_capacity(const double *snr_db, int n, double *out);
int polar_ga_phi_tables(double phi_dx, double *fwd, double *inv);
int polar_polarized_counts(int constellation, const double *snr_db, int n, long num_sym, uint64_t seed, uint64_t trial0,
                           uint64_t *counts);
int polar_polarized_capacity_from_counts(int constellation, int n, const uint64_t *counts, double *out);
int polar_polarized_capacity(int constellation, const double *snr_db, int n, long num_sym, uint64_t seed, double *out);
int polar_ga_mean_llr(const double *capacity, int n, double *mean_llr);
int polar_ga_construction(int n, int constellation, const double *snr_db, int n_points, double phi_dx, uint64_t seed,
                          const double *capacity, double *channels, uint16_t *order, double *bler_prefix);

/* tuning knobs (0 = default): waves resident per CU and LDS-resident layer exponent */
int polar_set_tuning(polar_code_t *h, int waves_per_cu, int lds_log);
/* node arithmetic of decode_scl_llr: 0 = automatic (exp-domain kernel for list sizes >= 3, LLR-domain kernel
 * below), 1 = LLR-domain kernel only (table-driven exp/log1p f-node, the round-1 path), 2 = exp-domain kernel
 * (f-node = one division; codewords it cannot decide safely are flagged on the device and decoded again by the
 * LLR-domain kernel in the same call).
 * Decoded bits are the reference's in every mode for codes a construction produces for its channel (every BASELINE
 * configuration, the golden vectors, the fuzz slice of the -m gpu suite). Where unfrozen leaves lie in the worst synthetic
 * channels (explicit tables, rates near 1) the reference itself decides on the rounding noise of glibc's exp/log, which no
 * other arithmetic reproduces bit for bit: the handle marks such leaves at creation (BEC(1/2) capacity below 1e-3) and every
 * codeword in which one of them comes out below 1e-8 is decoded by the LLR-domain kernel whatever the mode, so automatic
 * mode is never worse there than mode 1 (HISTORY.md "Where bit-exactness ends"; tests/test_gpu_fuzz.py). With list sizes
 * below 3 mode 2 falls back to the LLR-domain kernel (the exp-domain kernels exist for groups of 4 lanes and more).
 * Environment overrides (measurement and tests only) are read ONCE, when a handle is created, and validated — no entry
 * point calls getenv afterwards: POLAR_MODE=<0|1|2> replaces the handle's mode (any other value: creation fails);
 * POLAR_SC_NO_FOLD=1 makes the list-size-1 kernel decode a permuted, converted copy of the batch (its round-2 front pass)
 * instead of reading the caller's rows in place; POLAR_NO_TABLES=1, POLAR_NO_HEAD=1, POLAR_NO_RCCL=1, POLAR_FORCE_RCCL=1. Results do not
 * depend on any of them. */
int polar_set_mode(polar_code_t *h, int mode);
/* how many unfrozen leaves the handle classified as weak at creation (BEC(1/2) capacity below 1e-3; see above). Codes with
 * weak leaves are accepted, but their decoded bits are the reference's only as far as the LLR-domain kernel reproduces
 * glibc's rounding noise: polar_create_explicit() reports POLAR_W_WEAK_LEAVES (a positive, non-error status; the handle is
 * valid) and this function the count. */
int polar_get_weak_leaves(const polar_code_t *h);
/* Measurement knobs and test hooks (polar_debug_set / polar_debug_get / ...) are NOT part of this interface: they are declared
 * in include/polar_amd_debug.h, and the fault-injection hooks among them exist only in the test build of the library. */

#ifdef __cplusplus
}
#endif
#endif /* POLAR_AMD_H */
