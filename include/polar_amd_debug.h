/* polar_amd_debug.h — measurement knobs and test hooks of libpolar_amd.so. NOT part of the drop-in interface
 * (include/polar_amd.h does not include this file; nothing here has a counterpart in the reference's PolarCode class):
 * tools/, bench.py's diagnostic records and tests/ use it.
 *
 * Two libraries are built from the same sources (polar_amd/build.py):
 *   libpolar_amd.so       the product: the MEASUREMENT knobs below only. A fault-injection key is an unknown key.
 *   libpolar_amd_test.so  the same code compiled with -DPOLAR_TEST_HOOKS: additionally the FAULT-INJECTION keys, which make a
 *                         Monte-Carlo sweep fail, stall or share a device on purpose (tests of the failure protocol and of the
 *                         multi-device paths on a single-GPU box load this one).
 */
#ifndef POLAR_AMD_DEBUG_H
#define POLAR_AMD_DEBUG_H
#include "polar_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* polar_debug_set(h, key, value): negative return = error (unknown key, value out of range).
 * Measurement knobs (both libraries; results never depend on them):
 *   "mode_override" -1|0|1|2      replaces polar_set_mode's value (-1 = none); POLAR_MODE in the environment at creation
 *   "sc_no_fold", "no_tables", "no_fuse_front", "no_prefix"     alternative (older) forms of single passes, for A/B timing
 *   "no_head"                     lists of 17 .. 32 in one phase: no 4-lane head in front of the list kernel (POLAR_NO_HEAD at creation)
 *   "no_r1"                       control words without the rate-1 block field: the list-of-32 kernels take every leaf of such a block as a step of its own (POLAR_NO_R1 at creation)
 *   "head_min_b"                  smallest batch that takes the head (0 = default: from 16 codewords per resident wave on)
 *   "no_rccl", "force_rccl"       counter reduction of the single-process multi-device driver (drops its cached context)
 *   "lat_max_b"                   largest batch that takes the one-codeword-per-wave kernels (0 = default, -1 = never)
 *   "lat_grid"                    at most this many blocks in a launch of those kernels (0 = default: what the device holds); a wave
 *                                 then decodes further codewords in turn, whatever the device's CU count
 *   "lane_grid"                   at most this many blocks in a codeword-per-lane launch of decode_scl_p1 / decode_sc_p1 / decode_mlc (and
 *                                 the MLC sweep); 0 = default: 16 waves per CU. The per-wave scratch is sized for the capped grid, and a
 *                                 wave then decodes further codewords in turn on the same scratch
 *   "host_pipe_min_bytes", "host_chunk_bytes", "host_lanes", "host_threads", "host_ramp", "host_prefault"
 *                                 the pipelined host-pointer path (0 = default everywhere)
 *   "list_chunk_cw"               codewords per output chunk of polar_decode_scl_llr_list_batch (0 = default: 256 MiB of list output)
 *   "multi_timeout_s", "multi_grace_s"    watchdog of a multi-device step and its grace periods
 * Fault injection (libpolar_amd_test.so only; no environment form):
 *   "share_device"                one GPU may be listed several times in a device list (separate contexts, host-side sum)
 *   "force_workers"               worker threads (and so the watchdog) even with one device
 *   "fail_device" = d, "fail_collective" = d    worker d fails in its second step before / after the barrier (-1 = off)
 *   "stall_device" = d, "stall_ms"              worker d sleeps in its second step before it launches anything
 * Like every entry point, the hooks must not run concurrently with another call on the same handle. Every setter drops
 * the handle's per-device contexts and extra decode lanes (they carry a copy of the knobs). */
int polar_debug_set(polar_code_t *h, const char *key, long value);
/* polar_debug_get(h, key): "allocs" (hipMalloc calls of all handles' scratch so far), "comm_inits", "weak_leaves",
 * "mode_override", "head_phi" (hand-over leaf of the handle's last decode_scl_llr launch, 0 = decoded in one phase),
 * "lat_waves" (blocks of the one-codeword-per-wave launch of the handle's last decode_scl_llr / decode_sc_p1 / decode_mlc call, 0 = it
 * took no such kernel, or was a pipelined host-pointer call, whose chunks are decoded on contexts of their own), "lane_waves" (blocks of
 * the codeword-per-lane launch of the handle's last decode_scl_p1 / decode_sc_p1 / decode_mlc call, 0 = it launched none), "scan_grid_cap" (most blocks of a polar_decode_scan_batch launch; its waves loop over the rest of the rows), "last_rounds", "last_round_max_per_device", "worker_threads_started", "multi_poisoned",
 * "round_us_first|min|median|max|count" (steps of the handle's last sweep), "host_chunks", "host_chunk_cw", "host_lanes",
 * "host_threads", "host_us_copy_in|wait|copy_out|total" (the last pipelined host-pointer call), "test_hooks" (1 in the test
 * build); -1 = unknown key. Test build only: "head_check" reads the hand-over records of the handle's last two-phase decode back
 * and returns how many codewords did not arrive with the planned paths (0 = the premise holds; -2 = no records to read). */
long polar_debug_get(const polar_code_t *h, const char *key);
/* Which codewords the handle's last decode_scl_llr call on device pointers handed to its fallback pass (the fast kernels flag the rows
 * whose decisions they cannot guarantee; the LLR-domain kernel decodes those again: DESIGN.md "Which rows take the fallback pass").
 * Synchronises the call's stream, copies min(count, cap) row indices (in no particular order) to `rows` and returns the count.
 * -1: the last call had no fallback pass (the LLR-domain families: lists of 1 with a path metric and of 2, mode 1; a pipelined
 * host-pointer call; no call yet). Below -1: -(1 + the hipError_t that stopped it). The buffers are the handle's: the answer is
 * valid until the next call on the handle. Both libraries. */
long polar_debug_fallback_rows(polar_code_t *h, uint32_t *rows, long cap);
/* The alive lists of the step-wise Monte-Carlo engine (polar_mc_batch, polar_mc_batch_ber, polar_mc_batch_bicm): the two buffers of
 * trial indices that the points of a round hand to one another (the trials that failed at a point are the ones simulated at the next
 * enabled point of the same list size). Copies min(count, cap) entries of buffer `which` (0 or 1), in no particular order, to `out`
 * and returns the count; -1: the handle has no such buffers (no round yet), or `which` is neither; below -1: -(1 + hipError_t). After
 * a round the two buffers hold what the last list size with an enabled point left: the failures of its last enabled point in one,
 * what that point was given (the failures of the enabled point before it, or all T trials if it was the only one) in the other.
 * Reads only; valid until the next call on the handle. Both libraries. */
long polar_debug_mc_alive(polar_code_t *h, int which, uint64_t *out, long cap);
/* The per-leaf control words as uploaded (marked != 0: with the rate-1 block field in bits 9-10, else the plain array the knob
 * "no_r1" selects): copies min(N, cap) words, returns N; below 0: -(1 + hipError_t). Both libraries. polar_debug_get
 * "r1_committed" / "r1_discarded" (test build only): the rate-1 quad continuations the last list-of-32 launch of the handle's
 * last call finished in one step / gave up, counted per wave: "committed" = quads finished whose own first leaf passed its test (a
 * chained second quad of an octet included), "discarded" = continuations tried in the loop after a fast first leaf and given up.
 * "r1_rank_tried" / "r1_rank_committed": continuations entered after a first leaf that took the ranking path; "r1_chain_tried" /
 * "r1_chain_committed": second quads of marked octets tried / finished in the step that finished the first. */
long polar_debug_ctl_words(polar_code_t *h, uint32_t *words, long cap, int marked);
/* number of ncclCommInitAll calls made by this library so far (the communicators of a device list are cached on the handle) */
int polar_debug_comm_inits(void);
/* older name of polar_get_weak_leaves (include/polar_amd.h) */
int polar_debug_weak_leaves(const polar_code_t *h);
/* instrumented development builds (POLAR_DEFS, polar_amd/build.py): where their kernels leave their counters */
void *polar_debug_scratch_ptr(polar_code_t *h);

#ifdef __cplusplus
}
#endif
#endif /* POLAR_AMD_DEBUG_H */
