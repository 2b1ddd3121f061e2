// polar_kernels_adapt.hip — the counters of the adaptive sweep (polar_mc_batch_adaptive). A unit of its own: the
// kernels of polar_kernels_metric.hip and polar_channel.hip keep their machine code only while those units stay as they are.
//
// The decode stages themselves are scl_decode_llr_adapt_kernel (polar_kernels.hip, POLAR_ED_TU = 7); the work lists between them come
// from ed_collect_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "polar_kernels.h"
#include "polar_wave_frame.h"

namespace {

constexpr int kMaxStages = 8;          // include/polar_amd.h POLAR_AD_MAX_STAGES

// One wave per codeword: the delivered word against the sent one. ctr[0] runs, [1] block errors (out != sent), [2] undetected errors
// (an error delivered with crc_ok = 1), [3 + s] codewords delivered by stage s. A wave counts its codewords in registers and adds
// once per class.
__global__ __launch_bounds__(64) void adapt_classify_kernel(const uint8_t *out, const uint8_t *stage, const uint8_t *crc_ok,
                                                             const uint8_t *sent, long B, int K, int n_s, unsigned long long *ctr) {
    const int lane = threadIdx.x;
    unsigned long long run = 0, err_n = 0, undet_n = 0, st_n[kMaxStages] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long c = blockIdx.x; c < B; c += gridDim.x) {
        const uint8_t *got = out + (size_t)c * K, *want = sent + (size_t)c * K;
        const bool err = rows_differ(got, want, K, lane);
        const int s = stage[c];
        run += 1; err_n += err; undet_n += (err && crc_ok[c] == 1);
#pragma unroll
        for (int k = 0; k < kMaxStages; ++k) st_n[k] += (s == k);
    }
    if (lane == 0) {
        if (run) atomicAdd(ctr + 0, run);
        if (err_n) atomicAdd(ctr + 1, err_n);
        if (undet_n) atomicAdd(ctr + 2, undet_n);
#pragma unroll
        for (int k = 0; k < kMaxStages; ++k)
            if (k < n_s && st_n[k]) atomicAdd(ctr + 3 + k, st_n[k]);
    }
}

}  // namespace

hipError_t polar_launch_adapt_classify(const uint8_t *out, const uint8_t *stage, const uint8_t *crc_ok, const uint8_t *sent, long B,
                                       int K, int n_s, unsigned long long *ctr, hipStream_t st) {
    if (n_s < 1 || n_s > kMaxStages) return hipErrorInvalidValue;
    hipLaunchKernelGGL(adapt_classify_kernel, dim3(polar_rows_grid(B)), dim3(64), 0, st, out, stage, crc_ok,
                       sent, B, K, n_s, ctr);
    return hipGetLastError();
}
