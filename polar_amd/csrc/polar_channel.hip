// polar_channel.hip — the front of the hot path on the device: encoder
// (PolarCode::encode, PolarCode.cpp:60-91), the synthetic BPSK/AWGN channel + LLR
// (PolarCode.cpp:703-716, 744-753 with the counter-based generator of
// include/polar_synth.h) and the error counter (PolarCode.cpp:758-769).
//
// One wavefront per codeword, the N message bits staged as bytes in LDS; HBM-bound byte work
// (N*8 B of LLR written per codeword), no MFMA.  Must be built with -ffp-contract=off: the
// LLRs have to be bit-identical to the host evaluation of polar_synth.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "polar_kernels.h"
#include "polar_synth.h"

namespace {

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// u[order[i]] = info[i]; crc bits; XOR butterfly: PolarCode.cpp:65-83. `u` is N bytes of LDS.
__device__ void encode_in_lds(volatile uint8_t *u, const uint8_t *info_lds, const PolarEncodeParams &p, int lane) {
    const int n = p.n, N = p.N, K = p.K;
    for (int i = lane; i < N; i += 64) u[i] = 0;
    wave_sync();
    for (int i = lane; i < K; i += 64) u[p.order[i]] = info_lds[i];
    for (int r = 0; r < p.crc; ++r) {
        unsigned par = 0;
        for (int j = lane; j < K; j += 64) par ^= (unsigned)(p.crcm[(size_t)r * K + j] & info_lds[j]);
        unsigned long long b = __ballot(par & 1u);
        if (lane == 0) u[p.order[K + r]] = (uint8_t)(__popcll(b) & 1);
    }
    wave_sync();
    for (int it = 0; it < n; ++it) {
        const int inc = 1 << it;
        for (int q = lane; q < N / 2; q += 64) {
            int a = ((q >> it) << (it + 1)) | (q & (inc - 1));
            u[a] = (uint8_t)(u[a] ^ u[a + inc]);
        }
        wave_sync();
    }
}

__global__ __launch_bounds__(64) void encode_kernel(PolarEncodeParams p) {
    extern __shared__ uint8_t sm[];
    volatile uint8_t *u = sm;          // [N]
    uint8_t *inf = sm + p.N;           // [K]
    const int lane = threadIdx.x;
    const long Bv = p.n_dev ? ((long)*p.n_dev < p.B ? (long)*p.n_dev : p.B) : p.B;
    for (long b = blockIdx.x; b < Bv; b += gridDim.x) {
        for (int i = lane; i < p.K; i += 64) inf[i] = p.info[(size_t)b * p.K + i];
        wave_sync();
        encode_in_lds(u, inf, p, lane);
        // coded[i] = u[bitrev[i]]: PolarCode.cpp:85-87
        for (int i = lane; i < p.N; i += 64) p.coded[(size_t)b * p.N + i] = u[__brev((unsigned)i) >> (32 - p.n)];
        wave_sync();
    }
}

__global__ __launch_bounds__(64) void synth_kernel(PolarEncodeParams p) {
    extern __shared__ uint8_t sm[];
    volatile uint8_t *u = sm;
    uint8_t *inf = sm + p.N;
    const int lane = threadIdx.x;
    const long Bv = p.n_dev ? ((long)*p.n_dev < p.B ? (long)*p.n_dev : p.B) : p.B;
    for (long b = blockIdx.x; b < Bv; b += gridDim.x) {
        const uint64_t trial = p.sel ? p.sel[b] : (p.trial0 + (uint64_t)b * (uint64_t)p.stride);
        const uint64_t block = trial / (uint64_t)p.info_block_div;   // 100: info refreshed every 100 runs, PolarCode.cpp:703-707
        for (int i = lane; i < p.K; i += 64) {
            uint32_t r[4];
            polar_synth_info_word(p.seed, block, (uint32_t)(i >> 7), r);
            int k = i & 127;
            inf[i] = (uint8_t)((r[(k >> 5) & 3] >> (k & 31)) & 1u);
        }
        wave_sync();
        if (p.info_out)
            for (int i = lane; i < p.K; i += 64) p.info_out[(size_t)b * p.K + i] = inf[i];
        encode_in_lds(u, inf, p, lane);
        if (p.coded)
            for (int i = lane; i < p.N; i += 64) p.coded[(size_t)b * p.N + i] = u[__brev((unsigned)i) >> (32 - p.n)];
        if (p.constellation != 0) {
            // ASK Gray + BICM demapper: Constellation.m:84-93, 123-144 (include/polar_synth.h)
            const int nb = polar_const_nbits(p.constellation);
            const int nsym = p.N / nb;
            double *dl = p.llr ? p.llr + (size_t)b * p.N : nullptr;
            if (dl)
                for (int i = nsym * nb + lane; i < p.N; i += 64) dl[i] = 0.0;
            for (int i = lane; i < nsym; i += 64) {
                int sym = 0;
                for (int j = 0; j < nb; ++j) sym += (1 << j) * (int)u[__brev((unsigned)(i * nb + j)) >> (32 - p.n)];
                const double x = polar_const_point(p.constellation, sym) / p.cnorm;
                const double y = x + polar_synth_symbol_noise(p.seed, trial, (uint32_t)i) * p.sigma;
                if (p.y_out) p.y_out[(size_t)b * nsym + i] = y;
                if (!dl) continue;
                double l4[4];
                polar_synth_bicm_demap(p.constellation, p.cnorm, y, p.n0, l4);
                for (int j = 0; j < nb; ++j) dl[(size_t)i * nb + j] = l4[j];
            }
            wave_sync();
            continue;
        }
        double2 *dst = reinterpret_cast<double2 *>(p.llr + (size_t)b * p.N);
        for (int pr = lane; pr < p.N / 2; pr += 64) {
            double z0, z1;
            polar_synth_noise_pair(p.seed, trial, (uint32_t)pr, &z0, &z1);
            int c0 = u[__brev((unsigned)(2 * pr)) >> (32 - p.n)];
            int c1 = u[__brev((unsigned)(2 * pr + 1)) >> (32 - p.n)];
            double2 v;
            v.x = polar_synth_llr(p.s, c0, z0);
            v.y = polar_synth_llr(p.s, c1, z1);
            dst[pr] = v;
        }
        wave_sync();
    }
}

// ---- the BICM demapper on its own (Constellation.m:123-144): received symbols -> interleaved LLR / p1 rows ----
// One lane per symbol, 256 symbols of a row per block, rows grid-strided over blockIdx.y. Per symbol 2^NB exponentials in
// symbol-index order and NB logarithms / divisions, all fp64 VALU work in registers (both loops unrolled: the label bit of
// (symbol, level) is a compile-time constant); the arithmetic is polar_synth_bicm_demap2's term for term — the same sums in
// the same order — with the normalised points taken from the launch parameters (computed once by the host with the same
// two correctly rounded operations). The loads are coalesced (consecutive lanes, consecutive symbols); the NB outputs of a
// lane are contiguous: 16-byte stores for 2 and 4 bits when the rows are 16-byte aligned (VEC), else one double per store
// (3 bits: 24 contiguous bytes per lane either way).
// one symbol: polar_synth_bicm_demap2 with the points given and the loops over a compile-time n_bits
template <int NB>
__host__ __device__ __forceinline__ void demap_symbol(const double *pt, double y, double n0, bool want_llr, double *l, double *q) {
    constexpr int NS = 1 << NB;
    double p0[NB], p1[NB];
#pragma unroll
    for (int m = 0; m < NB; ++m) { p0[m] = 0; p1[m] = 0; }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        double d = y - pt[s];
        double ad = d < 0 ? -d : d;
        double ps = polar_synth_exp_neg(-(ad * ad) / 2 / n0);
#pragma unroll
        for (int m = 0; m < NB; ++m) {
            if (((s >> m) & 1) == 0) p0[m] = p0[m] + ps; else p1[m] = p1[m] + ps;
        }
    }
#pragma unroll
    for (int m = 0; m < NB; ++m) {
        l[m] = want_llr ? polar_synth_log(p0[m] / p1[m]) : 0.0;
        q[m] = p1[m] / (p0[m] + p1[m]);
    }
}

template <int NB, typename T, bool VEC>
__global__ __launch_bounds__(256) void bicm_demap_kernel(PolarDemapParams p) {
    const long Bv = p.n_dev ? ((long)*p.n_dev < p.B ? (long)*p.n_dev : p.B) : p.B;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int tail = p.M * NB + (int)threadIdx.x;          // (N - M * NB < NB positions)
    const T *ys = static_cast<const T *>(p.y);
    for (long b = blockIdx.y; b < Bv; b += gridDim.y) {
        double *dl = p.llr ? p.llr + (size_t)b * p.N : nullptr;
        double *dp = p.p1 ? p.p1 + (size_t)b * p.N : nullptr;
        if (blockIdx.x == 0 && tail < p.N) {               // unused tail positions: p1 = 0.5 <=> llr = 0 (main_MC_CC_Comparison.m:94)
            if (dl) dl[tail] = 0.0;
            if (dp) dp[tail] = 0.5;
        }
        if (i >= p.M) continue;
        const double y = (double)ys[(size_t)b * p.M + i];  // (float -> double is exact)
        double l[NB], q[NB];
        demap_symbol<NB>(p.pt, y, p.n0, dl != nullptr, l, q);
        const size_t o = (size_t)i * NB;
        if constexpr (VEC && (NB == 2 || NB == 4)) {
#pragma unroll
            for (int m = 0; m < NB; m += 2) {
                if (dl) *reinterpret_cast<double2 *>(dl + o + m) = make_double2(l[m], l[m + 1]);
                if (dp) *reinterpret_cast<double2 *>(dp + o + m) = make_double2(q[m], q[m + 1]);
            }
        } else {
#pragma unroll
            for (int m = 0; m < NB; ++m) {
                if (dl) dl[o + m] = l[m];
                if (dp) dp[o + m] = q[m];
            }
        }
    }
}

template <int NB, typename T>
hipError_t launch_demap_nb(const PolarDemapParams &p, dim3 grid, bool vec, hipStream_t st) {
    if (vec) hipLaunchKernelGGL((bicm_demap_kernel<NB, T, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((bicm_demap_kernel<NB, T, false>), grid, dim3(256), 0, st, p);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_demap(const PolarDemapParams &p, dim3 grid, bool vec, hipStream_t st) {
    switch (p.nb) {
        case 1: return launch_demap_nb<1, T>(p, grid, false, st);
        case 2: return launch_demap_nb<2, T>(p, grid, vec, st);
        case 3: return launch_demap_nb<3, T>(p, grid, false, st);
        case 4: return launch_demap_nb<4, T>(p, grid, vec, st);
        default: return hipErrorInvalidValue;
    }
}

// one wave per codeword: any differing info bit => block error (PolarCode.cpp:758-769)
__global__ __launch_bounds__(64) void count_errors_kernel(const uint8_t *a, const uint8_t *b, long B, int K,
                                                           unsigned long long *err, uint8_t *flags) {
    const int lane = threadIdx.x;
    for (long c = blockIdx.x; c < B; c += gridDim.x) {
        bool diff = false;
        for (int i = lane; i < K; i += 64) diff |= (a[(size_t)c * K + i] != b[(size_t)c * K + i]);
        bool any = __any(diff);
        if (lane == 0) {
            if (any && err) atomicAdd(err, 1ull);
            if (flags) flags[c] = any ? 1 : 0;
        }
    }
}

// list output (polar_decode_scl_llr_list_batch_dev): in which row of its list is a given word? One wave per codeword, the lanes
// stride over the K bytes of a row, one ballot per row; rank_out[b] = the first row r < n_active[b] equal to info[b], or L
__global__ __launch_bounds__(64) void list_find_kernel(const uint8_t *cand, const int32_t *n_active, const uint8_t *info, long B, int L,
                                                        int K, int32_t *rank_out) {
    const int lane = threadIdx.x;
    for (long c = blockIdx.x; c < B; c += gridDim.x) {
        int na = n_active[c];
        na = na < 0 ? 0 : (na > L ? L : na);
        const uint8_t *want = info + (size_t)c * K;
        int found = L;
        for (int r = 0; r < na; ++r) {
            const uint8_t *row = cand + ((size_t)c * L + r) * (size_t)K;
            bool diff = false;
            for (int i = lane; i < K; i += 64) diff |= (row[i] != want[i]);
            if (__ballot(diff) == 0) { found = r; break; }        // (wave-uniform)
        }
        if (lane == 0) rank_out[c] = found;
    }
}

// ---- Monte-Carlo round, device side (no host round trip between the (L, Eb/N0) points) ----
__global__ __launch_bounds__(256) void mc_init_alive_kernel(uint64_t *alive, unsigned *n, uint64_t t0, long stride, long T) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < T; i += (long)gridDim.x * 256) alive[i] = t0 + (uint64_t)i * (uint64_t)stride;
    if (blockIdx.x == 0 && threadIdx.x == 0) *n = (unsigned)T;
}
__global__ __launch_bounds__(64) void mc_count_compact_kernel(const uint8_t *dec, const uint8_t *sent, long B, int K,
                                                               const uint64_t *alive_in, const unsigned *n_in, uint64_t *alive_out,
                                                               unsigned *n_out, unsigned long long *ctr) {
    const int lane = threadIdx.x;
    if (n_in && (long)*n_in < B) B = (long)*n_in;          // (n_in == nullptr: exactly B rows)
    for (long c = blockIdx.x; c < B; c += gridDim.x) {
        unsigned nd = 0;
        for (int i = lane; i < K; i += 64) nd += (dec[(size_t)c * K + i] != sent[(size_t)c * K + i]) ? 1u : 0u;
        for (int off = 32; off >= 1; off >>= 1) nd += __shfl_xor(nd, off, 64);
        if (lane == 0 && nd) {
            atomicAdd(ctr, 1ull);
            atomicAdd(ctr + 1, (unsigned long long)nd);
            alive_out[atomicAdd(n_out, 1u)] = alive_in[c];
        }
    }
}

}  // namespace

hipError_t polar_launch_encode(const PolarEncodeParams &p, hipStream_t st) {
    hipLaunchKernelGGL(encode_kernel, dim3(polar_rows_grid(p.B)), dim3(64), (size_t)p.N + p.K, st, p);
    return hipGetLastError();
}
hipError_t polar_launch_synth(const PolarEncodeParams &p, hipStream_t st) {
    hipLaunchKernelGGL(synth_kernel, dim3(polar_rows_grid(p.B)), dim3(64), (size_t)p.N + p.K, st, p);
    return hipGetLastError();
}
hipError_t polar_launch_bicm_demap(const PolarDemapParams &p, hipStream_t st) {
    if (p.nb < 1 || p.nb > 4 || p.M != p.N / p.nb || (!p.llr && !p.p1) || !p.y) return hipErrorInvalidValue;
    if (p.B <= 0) return hipSuccess;
    // (a row starts 16-byte aligned when the base is and N is even; symbol i of a 2- / 4-bit label then starts at a multiple of 16 bytes)
    const bool vec = (((uintptr_t)p.llr | (uintptr_t)p.p1) & 15u) == 0 && (p.N & 1) == 0;
    const dim3 grid((unsigned)std::max(1, (p.M + 255) / 256), (unsigned)polar_rows_grid(p.B));
    return p.y_f32 ? launch_demap<float>(p, grid, vec, st) : launch_demap<double>(p, grid, vec, st);
}
hipError_t polar_launch_mc_init_alive(uint64_t *alive, unsigned *n, uint64_t t0, long stride, long T, hipStream_t st) {
    const long blocks = (T + 255) / 256;
    hipLaunchKernelGGL(mc_init_alive_kernel, dim3((unsigned)(blocks < 1024 ? (blocks ? blocks : 1) : 1024)), dim3(256), 0, st, alive, n, t0, stride, T);
    return hipGetLastError();
}
hipError_t polar_launch_mc_count_compact(const uint8_t *decoded, const uint8_t *sent, long B, int K,
                                         const uint64_t *alive_in, const unsigned *n_in, uint64_t *alive_out, unsigned *n_out,
                                         unsigned long long *ctr, hipStream_t st) {
    hipLaunchKernelGGL(mc_count_compact_kernel, dim3(polar_rows_grid(B)), dim3(64), 0, st, decoded, sent, B, K, alive_in, n_in, alive_out, n_out, ctr);
    return hipGetLastError();
}
hipError_t polar_launch_count_errors(const uint8_t *a, const uint8_t *b, long B, int K,
                                     unsigned long long *err, uint8_t *flags, hipStream_t st) {
    hipLaunchKernelGGL(count_errors_kernel, dim3(polar_rows_grid(B)), dim3(64), 0, st, a, b, B, K, err, flags);
    return hipGetLastError();
}
hipError_t polar_launch_list_find(const uint8_t *cand, const int32_t *n_active, const uint8_t *info, long B, int L, int K,
                                  int32_t *rank_out, hipStream_t st) {
    hipLaunchKernelGGL(list_find_kernel, dim3(polar_rows_grid(B)), dim3(64), 0, st, cand, n_active, info, B, L, K, rank_out);
    return hipGetLastError();
}
