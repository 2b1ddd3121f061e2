// polar_kernels_mlc.hip — the multi-level coding (MLC) receiver of PolarM (main_MC_CC_Comparison.m:55-62, 98-110;
// PolarCode.m:155-161, 180-190) for set-partition (and Gray) ASK: nb component polar codes of length M = N / nb, component k
// carried by label bit k of the symbols, decoded in stages — layer k is demapped conditioned on the re-encoded decisions of
// layers 0..k-1 (Constellation.m:95-121), SC-decoded in the probability domain (PolarCode.m:870-895) and re-encoded up to
// the root for the next stage. Workload definition and demapper: include/polar_synth.h.
//
//   mlc_front_kernel   — one wave per trial: message (sweep info or construction bits), per-component XOR butterfly in LDS,
//                        set-partition mapping, AWGN; writes the symbols [B][M] (and the sent info / packed message bits).
//                        Follows the alive-list indirection of synth_kernel (polar_channel.hip).
//   mlc_sc_kernel      — the multistage SC decoder, one LANE per codeword, state in a per-wave scratch [elem][lane] (batches).
//   mlc_sc_lat_kernel  — the same decoder with ONE codeword per wave, elements over the lanes, all state in LDS (small batches).
//   mlc_genie_kernel   — the genie-aided multistage decoder of the Monte-Carlo construction: each layer conditioned on the TRUE
//                        coded bits of the layers below, per-position error ballot + atomic as mc_genie_kernel (layer-major).
//
// Node expressions, element order (bit-reversed layers: a node combines elements j and j+S) and the leaf rule are those of
// sc_p1_kernel / sc_p1_lat_kernel / mc_genie_kernel (polar_kernels_p1.hip, polar_construct.hip) character for character; the
// root that those kernels stop short of (4*S > N) is completed here: root element j = cnop(xl[M/2 + j], xr[M/2 + j]),
// element j + M/2 = xr[M/2 + j], natural index i at element brev(i). Build with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "polar_kernels.h"
#include "polar_device.h"
#include "polar_synth.h"

namespace {

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ long rows_of(const PolarMlcParams &p) {
    return p.n_dev ? ((long)*p.n_dev < p.B ? (long)*p.n_dev : p.B) : p.B;
}

__global__ __launch_bounds__(64) void mlc_front_kernel(PolarMlcParams p, int mode) {
    extern __shared__ uint8_t sm[];
    volatile uint8_t *u = sm;                 // [N] message, then the nb component codewords (butterfly order)
    const int lane = threadIdx.x;
    const int N = p.N, K = p.K, m = p.m, M = p.M, nb = p.nb;
    const int words = (N + 31) / 32;
    const long Bv = rows_of(p);
    for (long b = blockIdx.x; b < Bv; b += gridDim.x) {
        const uint64_t trial = p.sel ? p.sel[b] : (p.trial0 + (uint64_t)b * (uint64_t)p.stride);
        if (mode == 1) {
            // construction: N random message bits, layer-major (PolarCode.m:157: rand(num_codes, N/num_codes) < 0.5)
            for (int q = lane; q < words; q += 64) {
                uint32_t r[4];
                polar_synth_mc_info_word(p.seed, trial, (uint32_t)(q >> 2), r);
                uint32_t w = r[q & 3];
                if (N < 32) w &= (1u << N) - 1u;
                p.minfo[(size_t)b * words + q] = w;
                for (int j = 0; j < 32 && 32 * q + j < N; ++j) u[32 * q + j] = (uint8_t)((w >> j) & 1u);
            }
        } else {
            // info_paded(info_bits) = info (main_MC_CC_Comparison.m:58-59)
            for (int i = lane; i < N; i += 64) u[i] = 0;
            wave_sync();
            for (int i = lane; i < K; i += 64) {
                uint8_t bit;
                if (p.info) bit = p.info[(size_t)b * K + i];
                else {
                    uint32_t r[4];
                    polar_synth_info_word(p.seed, trial / (uint64_t)p.info_block_div, (uint32_t)(i >> 7), r);
                    const int k = i & 127;
                    bit = (uint8_t)((r[(k >> 5) & 3] >> (k & 31)) & 1u);
                }
                u[p.order[i]] = bit;
                if (p.info_out) p.info_out[(size_t)b * K + i] = bit;
            }
        }
        wave_sync();
        // polar_encode of every component (:60-61): in-place XOR butterfly within each M-slice, read out bit-reversed
        for (int it = 0; it < m; ++it) {
            const int inc = 1 << it;
            for (int q = lane; q < N / 2; q += 64) {
                const int c = q >> (m - 1), ql = q & (M / 2 - 1);
                const int a = c * M + (((ql >> it) << (it + 1)) | (ql & (inc - 1)));
                u[a] = (uint8_t)(u[a] ^ u[a + inc]);
            }
            wave_sync();
        }
        // coded_bits(layer:num_codes:N) = component `layer` (:61); modulate (Constellation.m:84-93): symbol i = sum 2^k bit k
        for (int i = lane; i < M; i += 64) {
            const int br = (int)(__brev((unsigned)i) >> (32 - m));
            int sym = 0;
            for (int k = 0; k < nb; ++k) {
                const int bit = u[k * M + br];
                sym += (1 << k) * bit;
                if (p.coded) p.coded[(size_t)b * N + (size_t)i * nb + k] = (uint8_t)bit;
            }
            if (p.y) {
                const double x = polar_const_point(p.constellation, sym) / p.cnorm;
                p.y[(size_t)b * M + i] = x + polar_synth_symbol_noise(p.seed, trial, (uint32_t)i) * p.sigma;   // :88-92
            }
        }
        wave_sync();
    }
}

__device__ __forceinline__ uint8_t decision_byte(double x) { return x == 0.0 ? (uint8_t)0 : (x == 1.0 ? (uint8_t)1 : (uint8_t)2); }

// ---- multistage SC, one lane per codeword ------------------------------------------------------------------------------
// per-wave scratch [elem][lane]: y layers (size S at offset S), xl / xr (same offsets), p1 of the layer being decoded [M],
// the re-encoded decisions of the lower layers [(nb-1)*M] (natural order), the leaf decisions of every layer u[N]
__global__ __launch_bounds__(64) void mlc_sc_kernel(PolarMlcParams p) {
    const int lane = threadIdx.x;
    const int n = p.m, N = p.M, K = p.K, nb = p.nb;
    const size_t per = (size_t)(4 * N + (nb - 1) * N + p.N);
    double *gy = p.scr + (size_t)blockIdx.x * per * 64;
    double *gxl = gy + (size_t)N * 64;
    double *gxr = gxl + (size_t)N * 64;
    double *gp = gxr + (size_t)N * 64;
    double *gc = gp + (size_t)N * 64;
    double *gu = gc + (size_t)(nb - 1) * N * 64;
    const long Bv = rows_of(p);
    for (long c0 = (long)blockIdx.x * 64; c0 < Bv; c0 += (long)gridDim.x * 64) {
        const long cw = c0 + lane;
        if (cw < Bv) {
            const double *ys = p.y + (size_t)cw * N;
            for (int k = 0; k < nb; ++k) {
                // p1 = compute_llr_mlc(y, sigma^2, decoded_coded(:, 1:layer-1)) (main_MC_CC_Comparison.m:103)
                for (int i = 0; i < N; ++i) {
                    double ul[4];
                    for (int q = 0; q < k; ++q) ul[q] = gc[(size_t)(q * N + i) * 64 + lane];
                    double v;
                    polar_synth_mlc_demap(p.constellation, p.cnorm, ys[i], p.n0, k, ul, &v, nullptr);
                    gp[(size_t)i * 64 + lane] = v;
                }
                // [decoded_info(:, layer), decoded_coded(:, layer)] = polar_decode(p1, frozen_bits(slice)) (:105)
                const uint8_t *fz = p.frozen + (size_t)k * N;
                double *gk = gu + (size_t)k * N * 64;
                for (int phi = 0; phi < N; ++phi) {
                    const int lam_top = phi ? (n - __builtin_ctz((unsigned)phi)) : 1;
                    double leaf = 0.0;
                    for (int lam = lam_top; lam <= n; ++lam) {
                        const int sh = n - lam, S = 1 << sh;
                        const bool odd = (phi >> sh) & 1;
                        for (int j = 0; j < S; ++j) {
                            double a, b;
                            if (lam == 1) {
                                unsigned idx = __brev((unsigned)j) >> (32 - n);
                                a = gp[(size_t)idx * 64 + lane]; b = gp[(size_t)(idx + 1) * 64 + lane];
                            } else {
                                a = gy[(size_t)(2 * S + j) * 64 + lane];
                                b = gy[(size_t)(2 * S + j + S) * 64 + lane];
                            }
                            double r;
                            if (!odd) r = a * (1 - b) + b * (1 - a);                       // cnop, PolarCode.m:889-891
                            else {
                                const double x = gxl[(size_t)(S + j) * 64 + lane];
                                const double w1 = x * (1 - a) + a * (1 - x);                // cnop(u1hardprev, y_odd)
                                r = w1 * b / (w1 * b + (1 - w1) * (1 - b));                 // vnop, :893-895
                            }
                            gy[(size_t)(S + j) * 64 + lane] = r;
                            leaf = r;
                        }
                    }
                    double x;
                    if (fz[phi]) x = 0.0;                                                    // :875-876
                    else { const double tt = 1 - 2 * leaf; x = (1 - (double)((tt > 0) - (tt < 0))) / 2; }   // :873
                    gk[(size_t)phi * 64 + lane] = x;
                    if ((phi & 1) == 0) gxl[(size_t)1 * 64 + lane] = x;
                    else {
                        gxr[(size_t)1 * 64 + lane] = x;
                        int S = 1, ph = phi;
                        for (;;) {
                            if (4 * S > N) break;
                            const int psi = ph >> 1;
                            const bool to_right = psi & 1;
                            double *dst = (to_right ? gxr : gxl) + (size_t)(2 * S) * 64 + lane;
                            for (int j = 0; j < S; ++j) {
                                const double x1 = gxl[(size_t)(S + j) * 64 + lane], x2 = gxr[(size_t)(S + j) * 64 + lane];
                                dst[(size_t)j * 64] = x1 * (1 - x2) + x2 * (1 - x1);         // cnop(u1hard,u2hard) :885
                                dst[(size_t)(j + S) * 64] = x2;
                            }
                            if (!to_right) break;
                            S *= 2; ph = psi;
                        }
                    }
                }
                // the root: x = reshape([cnop(u1hardprev, u2hardprev); u2hardprev], 1, []) (:885), natural order
                if (k + 1 < nb)
                    for (int i = 0; i < N; ++i) {
                        const int s = (int)(__brev((unsigned)i) >> (32 - n));
                        double x;
                        if (s < N / 2) {
                            const double x1 = gxl[(size_t)(N / 2 + s) * 64 + lane], x2 = gxr[(size_t)(N / 2 + s) * 64 + lane];
                            x = x1 * (1 - x2) + x2 * (1 - x1);
                        } else x = gxr[(size_t)s * 64 + lane];
                        gc[(size_t)(k * N + i) * 64 + lane] = x;
                    }
            }
            // decoded_bits = u_decoded(info_bits) with u_decoded layer-major (:108-109)
            for (int b = 0; b < K; ++b) {
                const double x = gu[(size_t)p.order[b] * 64 + lane];
                if (p.out) p.out[(size_t)cw * K + b] = x;
                if (p.out_bytes) p.out_bytes[(size_t)cw * K + b] = decision_byte(x);
            }
        }
    }
}

// ---- the same decoder for SMALL batches: one codeword per wave, elements over the lanes, the whole state in LDS ------------
// LDS: y layers [M], xl / xr [M] each, p1 [M], re-encoded lower layers [(nb-1)*M], leaf decisions [N], frozen flags [N] bytes.
// The per-component SC is sc_p1_lat_kernel's (same expressions, same element order, no reductions): the doubles are
// mlc_sc_kernel's bit for bit.
__global__ __launch_bounds__(64) void mlc_sc_lat_kernel(PolarMlcParams p) {
    extern __shared__ double lds_mlc[];
    const int lane = threadIdx.x;
    const int n = p.m, N = p.M, K = p.K, nb = p.nb;
    double *ly = lds_mlc, *lxl = ly + N, *lxr = lxl + N, *lp = lxr + N, *lc = lp + N, *lu = lc + (nb - 1) * N;
    unsigned char *lfz = reinterpret_cast<unsigned char *>(lu + p.N);
    for (int i = lane; i < p.N; i += 64) lfz[i] = p.frozen[i];
    wave_mem_fence();
    const long Bv = rows_of(p);
    for (long cw = blockIdx.x; cw < Bv; cw += gridDim.x) {
        const double *ys = p.y + (size_t)cw * N;
        for (int k = 0; k < nb; ++k) {
            for (int i = lane; i < N; i += 64) {
                double ul[4];
                for (int q = 0; q < k; ++q) ul[q] = lc[q * N + i];
                double v;
                polar_synth_mlc_demap(p.constellation, p.cnorm, ys[i], p.n0, k, ul, &v, nullptr);
                lp[i] = v;
            }
            wave_mem_fence();
            const unsigned char *fzk = lfz + k * N;
            double *luk = lu + k * N;
            double xprev = 0.0;                                                          // decision of the pair's left leaf
            for (int phi = 0; phi < N; ++phi) {
                const bool fz = fzk[phi] != 0;
                const int lam_top = phi ? (n - __builtin_ctz((unsigned)phi)) : 1;
                const int lam_hi = (n > 1) ? n - 1 : n;
                for (int lam = lam_top; lam <= lam_hi; ++lam) {
                    const int sh = n - lam, S = 1 << sh;
                    const bool odd = (phi >> sh) & 1;
                    for (int j = lane; j < S; j += 64) {
                        double a, b;
                        if (lam == 1) {
                            const unsigned idx = __brev((unsigned)j) >> (32 - n);
                            a = lp[idx]; b = lp[idx + 1];
                        } else {
                            a = ly[2 * S + j]; b = ly[2 * S + j + S];
                        }
                        double r;
                        if (!odd) r = a * (1 - b) + b * (1 - a);                       // cnop, PolarCode.m:889-891
                        else {
                            const double x = lxl[S + j];
                            const double w1 = x * (1 - a) + a * (1 - x);                // cnop(u1hardprev, y_odd)
                            r = w1 * b / (w1 * b + (1 - w1) * (1 - b));                 // vnop, :893-895
                        }
                        ly[S + j] = r;
                    }
                    wave_mem_fence();
                }
                double leaf;
                if (n > 1) {
                    const double a = ly[2], b = ly[3];
                    if ((phi & 1) == 0) leaf = a * (1 - b) + b * (1 - a);
                    else {
                        const double w1 = xprev * (1 - a) + a * (1 - xprev);
                        leaf = w1 * b / (w1 * b + (1 - w1) * (1 - b));
                    }
                } else leaf = ly[1];
                double x;
                if (fz) x = 0.0;                                                         // :875-876
                else { const double tt = 1 - 2 * leaf; x = (1 - (double)((tt > 0) - (tt < 0))) / 2; }   // :873
                if (lane == 0) luk[phi] = x;
                if ((phi & 1) == 0) {
                    xprev = x;
                    if (n == 1) { if (lane == 0) lxl[1] = x; wave_mem_fence(); }
                } else if (4 <= N) {
                    int ph = phi >> 1;
                    bool to_right = ph & 1;
                    if (lane == 0) {
                        double *dst = (to_right ? lxr : lxl) + 2;
                        dst[0] = xprev * (1 - x) + x * (1 - xprev);
                        dst[1] = x;
                    }
                    wave_mem_fence();
                    int S = 2;
                    while (to_right && 4 * S <= N) {
                        const int psi = ph >> 1;
                        to_right = psi & 1;
                        double *dst = (to_right ? lxr : lxl) + 2 * S;
                        for (int j = lane; j < S; j += 64) {
                            const double x1 = lxl[S + j], x2 = lxr[S + j];
                            dst[j] = x1 * (1 - x2) + x2 * (1 - x1);                         // cnop(u1hard, u2hard) :885
                            dst[j + S] = x2;
                        }
                        wave_mem_fence();
                        S *= 2; ph = psi;
                    }
                }
            }
            wave_mem_fence();
            if (k + 1 < nb) {
                for (int i = lane; i < N; i += 64) {
                    const int s = (int)(__brev((unsigned)i) >> (32 - n));
                    // (at N = 2 the pair is the two leaf decisions: the first level above them is not stored at that size)
                    const double x1 = N == 2 ? luk[0] : lxl[N / 2 + (s & (N / 2 - 1))];
                    const double x2 = N == 2 ? luk[1] : lxr[N / 2 + (s & (N / 2 - 1))];
                    lc[k * N + i] = s < N / 2 ? x1 * (1 - x2) + x2 * (1 - x1) : x2;
                }
                wave_mem_fence();
            }
        }
        for (int b = lane; b < K; b += 64) {
            const double x = lu[p.order[b]];
            if (p.out) p.out[(size_t)cw * K + b] = x;
            if (p.out_bytes) p.out_bytes[(size_t)cw * K + b] = decision_byte(x);
        }
        wave_mem_fence();
    }
}

// ---- genie-aided multistage decoding of the Monte-Carlo construction (PolarCode.m:180-190, polar_decode_monte :897-914) ---
// one lane per run; per-wave scratch: y layers [M] + p1 [M] doubles, xl / xr [M] each + true coded bits of the lower layers
// [(nb-1)*M] bytes, all [elem][lane]
__global__ __launch_bounds__(64) void mlc_genie_kernel(PolarMlcParams p) {
    const int lane = threadIdx.x;
    const int n = p.m, N = p.M, nb = p.nb;
    const int words = (p.N + 31) / 32;
    double *gy = p.scr + (size_t)blockIdx.x * (size_t)(2 * N) * 64;
    double *gp = gy + (size_t)N * 64;
    uint8_t *gxl = p.x_scr + (size_t)blockIdx.x * (size_t)(2 * N + (nb - 1) * N) * 64;
    uint8_t *gxr = gxl + (size_t)N * 64;
    uint8_t *gc = gxr + (size_t)N * 64;
    for (long c0 = (long)blockIdx.x * 64; c0 < p.B; c0 += (long)gridDim.x * 64) {
        const long run = c0 + lane;
        const bool valid = run < p.B;
        const double *ys = p.y + (size_t)(valid ? run : 0) * N;
        const uint32_t *inf = p.minfo + (size_t)(valid ? run : 0) * words;
        for (int k = 0; k < nb; ++k) {
            // [p1, ~] = compute_llr_mlc(y, sigma^2, u) with u = the true coded bits of the layers below (:185-186)
            for (int i = 0; i < N; ++i) {
                double ul[4];
                for (int q = 0; q < k; ++q) ul[q] = (double)gc[(size_t)(q * N + i) * 64 + lane];
                double v;
                polar_synth_mlc_demap(p.constellation, p.cnorm, ys[i], p.n0, k, ul, &v, nullptr);
                gp[(size_t)i * 64 + lane] = v;
            }
            for (int phi = 0; phi < N; ++phi) {
                const int pos = k * N + phi;
                const unsigned ubit = (inf[pos >> 5] >> (pos & 31)) & 1u;
                const int lam_top = phi ? (n - __builtin_ctz((unsigned)phi)) : 1;
                double leaf = 0.0;
                for (int lam = lam_top; lam <= n; ++lam) {
                    const int sh = n - lam, S = 1 << sh;
                    const bool odd = (phi >> sh) & 1;
                    for (int j = 0; j < S; ++j) {
                        double a, b;
                        if (lam == 1) {
                            const unsigned idx = __brev((unsigned)j) >> (32 - n);
                            a = gp[(size_t)idx * 64 + lane]; b = gp[(size_t)(idx + 1) * 64 + lane];
                        } else {
                            a = gy[(size_t)(2 * S + j) * 64 + lane];
                            b = gy[(size_t)(2 * S + j + S) * 64 + lane];
                        }
                        double r;
                        if (!odd) {
                            r = a * (1 - b) + b * (1 - a);                            // cnop, PolarCode.m:889-891
                        } else {
                            const double w1 = gxl[(size_t)(S + j) * 64 + lane] ? 1 - a : a;
                            r = w1 * b / (w1 * b + (1 - w1) * (1 - b));                 // vnop, :893-895
                        }
                        gy[(size_t)(S + j) * 64 + lane] = r;
                        leaf = r;
                    }
                }
                const bool ok = (leaf > 0.5 && ubit == 1u) || (leaf <= 0.5 && ubit == 0u);     // :899-905
                const unsigned long long em = __ballot(valid && !ok);
                if (lane == 0 && em) atomicAdd(p.num_err + pos, (unsigned long long)__popcll(em));
                if ((phi & 1) == 0) gxl[(size_t)1 * 64 + lane] = (uint8_t)ubit;
                else {
                    gxr[(size_t)1 * 64 + lane] = (uint8_t)ubit;
                    int S = 1, ph = phi;
                    for (;;) {
                        if (4 * S > N) break;
                        const int psi = ph >> 1;
                        const bool to_right = psi & 1;
                        uint8_t *dst = (to_right ? gxr : gxl) + (size_t)(2 * S) * 64 + lane;
                        for (int j = 0; j < S; ++j) {
                            const uint8_t x1 = gxl[(size_t)(S + j) * 64 + lane], x2 = gxr[(size_t)(S + j) * 64 + lane];
                            dst[(size_t)j * 64] = (uint8_t)(x1 ^ x2);
                            dst[(size_t)(j + S) * 64] = x2;
                        }
                        if (!to_right) break;
                        S *= 2; ph = psi;
                    }
                }
            }
            // x of polar_decode_monte: the re-encoding of the true message (:912), natural order
            if (k + 1 < nb)
                for (int i = 0; i < N; ++i) {
                    const int s = (int)(__brev((unsigned)i) >> (32 - n));
                    const uint8_t x = s < N / 2 ? (uint8_t)(gxl[(size_t)(N / 2 + s) * 64 + lane] ^ gxr[(size_t)(N / 2 + s) * 64 + lane])
                                                : gxr[(size_t)s * 64 + lane];
                    gc[(size_t)(k * N + i) * 64 + lane] = x;
                }
        }
    }
}

}  // namespace

size_t polar_mlc_scr_doubles(int N, int nb) { return (size_t)(4 * (N / nb) + (nb - 1) * (N / nb) + N) * 64; }
size_t polar_mlc_lat_lds_bytes(int N, int nb) { return (size_t)(4 * (N / nb) + (nb - 1) * (N / nb) + N) * sizeof(double) + (size_t)N; }

hipError_t polar_launch_mlc_front(const PolarMlcParams &p, int mode, hipStream_t st) {
    const int grid = polar_rows_grid(p.B);
    hipLaunchKernelGGL(mlc_front_kernel, dim3(grid), dim3(64), (size_t)p.N, st, p, mode);
    return hipGetLastError();
}
hipError_t polar_launch_mlc_sc(const PolarMlcParams &p, int grid, hipStream_t st) {
    hipLaunchKernelGGL(mlc_sc_kernel, dim3(grid), dim3(64), 0, st, p);
    return hipGetLastError();
}
hipError_t polar_launch_mlc_sc_lat(const PolarMlcParams &p, int grid, hipStream_t st) {
    const size_t lds = polar_mlc_lat_lds_bytes(p.N, p.nb);
    // the kernel's dynamic-LDS limit is raised ONCE per device, to the device's per-block limit (not per launch: the sweep
    // launches this for every stage of every step); mlc_decode_launch only takes this kernel when `lds` fits that limit
    static std::atomic<unsigned long long> raised{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(raised.load(std::memory_order_acquire) & bit)) {
        int max_lds = 0;
        e = hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
        if (e != hipSuccess) return e;
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(mlc_sc_lat_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
        if (e != hipSuccess) return e;
        raised.fetch_or(bit, std::memory_order_release);
    }
    hipLaunchKernelGGL(mlc_sc_lat_kernel, dim3(grid), dim3(64), lds, st, p);
    return hipGetLastError();
}
hipError_t polar_launch_mlc_genie(const PolarMlcParams &p, int grid, hipStream_t st) {
    hipLaunchKernelGGL(mlc_genie_kernel, dim3(grid), dim3(64), 0, st, p);
    return hipGetLastError();
}
