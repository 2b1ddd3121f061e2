// polar_kernels_rm.hip — rate matching (include/polar_amd.h polar_rate_match_batch_dev, polar_rate_recover_batch_dev,
// polar_decode_scl_llr_rm_batch_dev, polar_synth_rm_llr_dev, polar_mc_batch_rm, polar_ga_construction_init).
//
//   rm_select_kernel    tx[b][e] = coded[b][sel[e]]: one lane per transmit position, the rows of the batch over grid.y.
//   rm_recover_kernel   the hot path: rx [B][E] -> llr fp64 [B][N]. The lanes are organised by OUTPUT position: a lane owns two
//                       adjacent coded positions of a row and loops over rows, so a wave stores 1 KiB of consecutive doubles per
//                       instruction (16 bytes a lane) and, for the schemes whose sel is contiguous, loads consecutive elements. The
//                       pattern arrives inverted (polar_rm.h): a lane reads its two descriptors ONCE, before its loop over the rows.
//                       No atomics, no LDS, plain vector stores. Per position acc = +0.0 (short_llr at a known one), then
//                       acc = acc + widen(rx[e]) in ascending e: the addition to +0.0 is kept (it turns -0.0 into +0.0, as the
//                       definition says); -ffp-contract=off and no reassociation.
//   rm_channel_kernel   the workload's channel over given transmit bits, one lane per noise pair (an odd E uses z0 of its last pair).
//   rm_classify_kernel  RUN / ERR / BIT of the sweep, one wave per codeword, one atomic per class and wave.
//   rm_ga_kernel        ga_construct_kernel of polar_kernels_ga.hip — the same expressions in the same order — with one block of N
//                       started from a per-position vector, and the forced leaves ranked behind all others in ascending index.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "polar_rm.h"
#include "polar_device.h"
#include "polar_synth.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRowsInFlight = 4;            // rows a lane has loads outstanding for

__global__ __launch_bounds__(kThreads) void rm_select_kernel(const uint8_t *coded, const uint16_t *sel, long B, int N, int E, uint8_t *tx) {
    const int e = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (e >= E) return;
    const unsigned src = sel[e];
    for (long b = blockIdx.y; b < B; b += gridDim.y) tx[(size_t)b * E + e] = coded[(size_t)b * N + src];
}

template <int FMT>
__device__ __forceinline__ double rm_load(const void *rx, size_t i) {
    if constexpr (FMT == 0) return reinterpret_cast<const double *>(rx)[i];
    else return llr_load_narrow(rx, i, FMT);
}
template <bool VEC>
__device__ __forceinline__ void rm_store(double *dst, double v0, double v1) {
    if constexpr (VEC) *reinterpret_cast<double2 *>(dst) = make_double2(v0, v1);
    else { dst[0] = v0; dst[1] = v1; }
}

// SINGLE: no position has more than one source (every pattern with E <= N and no repetition). tpr = lanes per row (a power of two,
// N / 2 at most), the block's other lanes take further rows
template <int FMT, bool SINGLE, bool VEC>
__global__ __launch_bounds__(kThreads) void rm_recover_kernel(PolarRmParams p, const void *rx, double *llr, int tpr) {
    const int t = threadIdx.x, rows_pb = kThreads / tpr;
    const int p0 = 2 * ((int)blockIdx.x * tpr + (t & (tpr - 1)));
    if (p0 >= p.N) return;
    const uint4 d = *reinterpret_cast<const uint4 *>(p.desc + 2 * (size_t)p0);
    const uint32_t c0 = d.x & ~kRmKnown, a0 = d.y, c1 = d.z & ~kRmKnown, a1 = d.w;
    const double f0 = (d.x & kRmKnown) ? p.short_llr : 0.0, f1 = (d.z & kRmKnown) ? p.short_llr : 0.0;
    const long step = (long)gridDim.y * rows_pb;
    const long b_first = (long)blockIdx.y * rows_pb + t / tpr;
    if constexpr (SINGLE) {
        for (long b = b_first; b < p.B; b += kRowsInFlight * step) {
            double v0[kRowsInFlight], v1[kRowsInFlight];
#pragma unroll
            for (int r = 0; r < kRowsInFlight; ++r) {
                const long bb = b + r * step;
                v0[r] = f0; v1[r] = f1;
                if (bb < p.B) {
                    const size_t row = (size_t)bb * (size_t)p.E;
                    if (c0) v0[r] = 0.0 + rm_load<FMT>(rx, row + a0);
                    if (c1) v1[r] = 0.0 + rm_load<FMT>(rx, row + a1);
                }
            }
#pragma unroll
            for (int r = 0; r < kRowsInFlight; ++r) {
                const long bb = b + r * step;
                if (bb < p.B) rm_store<VEC>(llr + (size_t)bb * (size_t)p.N + p0, v0[r], v1[r]);
            }
        }
    } else {
        for (long b = b_first; b < p.B; b += step) {
            const size_t row = (size_t)b * (size_t)p.E;
            double v0 = f0, v1 = f1;
            for (uint32_t k = 0; k < c0; ++k) v0 = v0 + rm_load<FMT>(rx, row + (c0 == 1 ? a0 : p.src[a0 + k]));
            for (uint32_t k = 0; k < c1; ++k) v1 = v1 + rm_load<FMT>(rx, row + (c1 == 1 ? a1 : p.src[a1 + k]));
            rm_store<VEC>(llr + (size_t)b * (size_t)p.N + p0, v0, v1);
        }
    }
}

__global__ __launch_bounds__(64) void rm_channel_kernel(const uint8_t *tx, long B, int E, uint64_t seed, uint64_t trial0, long stride,
                                                         double s, double *rx) {
    const int lane = threadIdx.x;
    for (long b = blockIdx.x; b < B; b += gridDim.x) {
        const uint64_t trial = trial0 + (uint64_t)b * (uint64_t)stride;
        const uint8_t *c = tx + (size_t)b * E;
        double *dst = rx + (size_t)b * E;
        for (int pr = lane; 2 * pr < E; pr += 64) {
            double z0, z1;
            polar_synth_noise_pair(seed, trial, (uint32_t)pr, &z0, &z1);
            dst[2 * pr] = polar_synth_llr(s, c[2 * pr], z0);
            if (2 * pr + 1 < E) dst[2 * pr + 1] = polar_synth_llr(s, c[2 * pr + 1], z1);
        }
    }
}

__global__ __launch_bounds__(64) void rm_classify_kernel(const uint8_t *dec, const uint8_t *sent, long B, int K, unsigned long long *ctr) {
    const int lane = threadIdx.x;
    unsigned long long cnt[3] = {0, 0, 0};
    for (long c = blockIdx.x; c < B; c += gridDim.x) {
        const size_t o = (size_t)c * K;
        unsigned nd = 0;
        for (int i = lane; i < K; i += 64) nd += (dec[o + i] != sent[o + i]) ? 1u : 0u;
        for (int off = 32; off >= 1; off >>= 1) nd += (unsigned)__shfl_xor((int)nd, off, 64);
        cnt[0] += 1; cnt[1] += nd != 0; cnt[2] += nd;
    }
    if (lane == 0)
        for (int k = 0; k < 3; ++k)
            if (cnt[k]) atomicAdd(ctr + k, cnt[k]);
}

// ---- construction: polar_kernels_ga.hip's phi_tab / phi_inv / ga_construct_kernel, expression for expression ----
constexpr int T = POLAR_GA_THREADS;

__device__ __forceinline__ double phi_tab(const double *fwd, double x) {
    x = x > 0 ? x : 0;
    x = x < 100 ? x : 100;
    return fwd[(int)round(x / 0.01)];
}
__device__ __forceinline__ double phi_inv(const unsigned long long *inv, double y) {
    double v = -polar_synth_log(y);
    v = v > 0 ? v : 0;
    v = v < 100 ? v : 100;
    return __longlong_as_double((long long)inv[(int)round(v / 1e-3 - 0.499)]);
}

__global__ __launch_bounds__(T) void rm_ga_kernel(PolarRmGaParams p) {
    __shared__ double part[T];
    const int pt = blockIdx.x, t = threadIdx.x;
    const int N = p.N;
    double *a = p.scr + (size_t)pt * 2 * N, *b = a + N;
    double *ch = p.channels + (size_t)pt * N;
    for (int i = t; i < N; i += T) a[i] = p.init[(size_t)pt * N + i];
    __syncthreads();
    for (int st = 0; st < p.n; ++st) {
        for (int q = t; q < N / 2; q += T) {
            const double c1 = a[2 * q], c2 = a[2 * q + 1];
            b[q] = phi_inv(p.inv, 1 - (1 - phi_tab(p.fwd, c1)) * (1 - phi_tab(p.fwd, c2)));
            b[N / 2 + q] = c1 + c2;
        }
        __syncthreads();
        double *tmp = a; a = b; b = tmp;
    }
    for (int i = t; i < N; i += T) ch[i] = a[(int)(__brev((unsigned)i) >> (32 - p.n))];
    __syncthreads();
    // stable descending sort of the leaves that are not forced; the forced ones behind them in ascending index
    uint16_t *ord = p.order + (size_t)pt * N;
    int n_forced = 0;
    if (p.forced)
        for (int j = 0; j < N; ++j) n_forced += p.forced[j] ? 1 : 0;
    for (int i = t; i < N; i += T) {
        const double c = ch[i];
        const bool fi = p.forced && p.forced[i];
        int rank = fi ? N - n_forced : 0;
        for (int j = 0; j < N; ++j) {
            const bool fj = p.forced && p.forced[j];
            const double d = ch[j];
            if (fi) rank += fj && j < i;
            else rank += !fj && ((d > c) || (d == c && j < i));
        }
        ord[rank] = (uint16_t)i;
    }
    __syncthreads();
    const int per = (N + T - 1) / T, lo = t * per, hi = min(N, lo + per);
    double s = 0.0;
    for (int r = lo; r < hi; ++r) s = s + 0.5 * erfc(sqrt(ch[min((int)ord[r], N - 1)]) / 2);
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        double acc = 0.0;
        for (int i = 0; i < T; ++i) { const double v = part[i]; part[i] = acc; acc = acc + v; }
    }
    __syncthreads();
    double *pre = p.prefix + (size_t)pt * N;
    double acc = part[t];
    for (int r = lo; r < hi; ++r) { acc = acc + 0.5 * erfc(sqrt(ch[min((int)ord[r], N - 1)]) / 2); pre[r] = acc; }
}

template <int FMT>
void recover_launch(const PolarRmParams &p, const void *rx, double *llr, hipStream_t st) {
    int tpr = 1;
    while (tpr < kThreads && 2 * tpr < p.N) tpr <<= 1;
    const int rows_pb = kThreads / tpr;
    const unsigned gx = (unsigned)((p.N / 2 + tpr - 1) / tpr);
    const long row_blocks = (p.B + rows_pb - 1) / rows_pb;
    const long cap = gx >= 16384 ? 1 : 16384 / gx;
    const dim3 grid(gx, (unsigned)(row_blocks < cap ? row_blocks : cap));
    const bool vec = ((uintptr_t)llr & 15u) == 0;
    const bool single = p.max_src <= 1;
    if (single && vec) hipLaunchKernelGGL((rm_recover_kernel<FMT, true, true>), grid, dim3(kThreads), 0, st, p, rx, llr, tpr);
    else if (single) hipLaunchKernelGGL((rm_recover_kernel<FMT, true, false>), grid, dim3(kThreads), 0, st, p, rx, llr, tpr);
    else if (vec) hipLaunchKernelGGL((rm_recover_kernel<FMT, false, true>), grid, dim3(kThreads), 0, st, p, rx, llr, tpr);
    else hipLaunchKernelGGL((rm_recover_kernel<FMT, false, false>), grid, dim3(kThreads), 0, st, p, rx, llr, tpr);
}

}  // namespace

hipError_t polar_launch_rm_select(const uint8_t *coded, const uint16_t *sel, long B, int N, int E, uint8_t *tx, hipStream_t st) {
    if (!coded || !sel || !tx || N < 2 || E < 1) return hipErrorInvalidValue;
    if (B <= 0) return hipSuccess;
    const dim3 grid((unsigned)((E + kThreads - 1) / kThreads), (unsigned)polar_rows_grid(B));
    hipLaunchKernelGGL(rm_select_kernel, grid, dim3(kThreads), 0, st, coded, sel, B, N, E, tx);
    return hipGetLastError();
}
hipError_t polar_launch_rm_recover(const PolarRmParams &p, const void *rx, int fmt, double *llr, hipStream_t st) {
    if (!rx || !llr || !p.desc || !p.src || p.N < 2 || (p.N & 1) || p.E < 1 || fmt < 0 || fmt > 3) return hipErrorInvalidValue;
    if (p.B <= 0) return hipSuccess;
    switch (fmt) {
        case 0: recover_launch<0>(p, rx, llr, st); break;
        case 1: recover_launch<1>(p, rx, llr, st); break;
        case 2: recover_launch<2>(p, rx, llr, st); break;
        default: recover_launch<3>(p, rx, llr, st); break;
    }
    return hipGetLastError();
}
hipError_t polar_launch_rm_channel(const uint8_t *tx, long B, int E, uint64_t seed, uint64_t trial0, long stride, double s, double *rx,
                                   hipStream_t st) {
    if (!tx || !rx || E < 1) return hipErrorInvalidValue;
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_channel_kernel, dim3(polar_rows_grid(B)), dim3(64), 0, st, tx, B, E, seed, trial0, stride, s, rx);
    return hipGetLastError();
}
hipError_t polar_launch_rm_classify(const uint8_t *dec, const uint8_t *sent, long B, int K, unsigned long long *ctr, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_classify_kernel, dim3(polar_rows_grid(B)), dim3(64), 0, st, dec, sent, B, K, ctr);
    return hipGetLastError();
}
hipError_t polar_launch_rm_ga_construct(const PolarRmGaParams &p, int n_points, hipStream_t st) {
    if (p.n < 1 || p.N != (1 << p.n) || n_points < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rm_ga_kernel, dim3(n_points), dim3(T), 0, st, p);
    return hipGetLastError();
}
