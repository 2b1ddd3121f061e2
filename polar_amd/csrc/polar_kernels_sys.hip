// polar_kernels_sys.hip — systematic polar coding (include/polar_amd.h polar_encode_sys_batch_dev, polar_sys_message_batch_dev,
// polar_sys_soft_batch_dev, polar_synth_sys_llr_dev, polar_mc_batch_sys).
//
// The precode and message kernels are bit-packed and register-resident: a codeword is W = max(1, N / 64) 64-bit words, bit p & 63 of
// word p >> 6 = position p of the encoder's natural order. Up to N = 4096 word w sits in lane w of the codeword's W lanes and 64 / W
// codewords share a wave; above, a lane holds R = W / 64 words, word w in register w >> 6 of lane w & 63. The butterfly stages
// u[a] ^= u[a + inc] are, for inc < 64, a shift, a mask and a xor inside every word; for inc >= 64 a xor with the word of another
// lane (__shfl_xor; the lanes whose word index has the stage's bit clear take it) or with another register of the same lane. The frozen
// mask, the CRC / syndrome rows and the D vectors of the parity positions are packed rows; a syndrome bit is the parity of the
// popcounts of an AND, all crc of them reduced across the codeword's lanes as ONE 32-bit word. Bytes come in through an inverse
// index table (position -> input byte) and one __ballot per word; they leave by testing bits of a word fetched from its lane with
// __shfl. No LDS, no barrier; every output is a plain vector store.
//
//   precode  x0 = pack(msg at msg_u); u = x0, `depth` times u = x0 ^ u ^ (mask & butterfly(u)); s = syndrome(u); zP = Q^-1 s;
//            u ^= sum zP[r] D_r; u_info = u at order; coded = butterfly(u) in bit-reversed order
//   message  u = pack(u_info at order), check bits from the CRC rows; z = butterfly(u); msg = z at msg_u
// The input rows of a wave's codewords are read completely (the pack) before any of their outputs is written: in place is safe.
//
// Beside them: the gather of the soft message outputs, the two halves of synth_kernel the systematic workload needs around the
// precode (the draw of the trials' info bits; the channel over GIVEN coded bits — the arithmetic of polar_channel.hip's synth_kernel,
// expression for expression, under -ffp-contract=off), and the classification of the sweep.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "polar_sys.h"
#include "polar_device.h"
#include "polar_synth.h"

namespace {

constexpr int kGridCap = 16384;

// positions whose bit `it` is clear, it = 0 .. 5
__device__ __forceinline__ u64 stage_mask(int it) {
    const u64 m[6] = {0x5555555555555555ull, 0x3333333333333333ull, 0x0F0F0F0F0F0F0F0Full,
                      0x00FF00FF00FF00FFull, 0x0000FFFF0000FFFFull, 0x00000000FFFFFFFFull};
    return m[it];
}

__device__ __forceinline__ u64 shfl_xor64(u64 v, int m) {
    const int lo = __shfl_xor((int)(unsigned)v, m, 64), hi = __shfl_xor((int)(unsigned)(v >> 32), m, 64);
    return ((u64)(unsigned)hi << 32) | (u64)(unsigned)lo;
}
__device__ __forceinline__ u64 shfl64(u64 v, int src) {
    const int lo = __shfl((int)(unsigned)v, src, 64), hi = __shfl((int)(unsigned)(v >> 32), src, 64);
    return ((u64)(unsigned)hi << 32) | (u64)(unsigned)lo;
}

// how the words of a wave's codewords are laid out: WL lanes a codeword (log2: wl_log), G codewords a wave
struct Layout {
    int W, WL, wl_log, G, g, wl;
};
template <int R>
__device__ __forceinline__ Layout make_layout(int N, int lane) {
    Layout y;
    y.W = N >= 64 ? N / 64 : 1;
    y.WL = y.W / R;
    y.wl_log = 31 - __clz(y.WL);
    y.G = 64 / y.WL;
    y.g = lane >> y.wl_log;
    y.wl = lane & (y.WL - 1);
    return y;
}

// the n stages of the encoder on the packed words (every lane of the wave takes part: the shuffles need all of them)
template <int R>
__device__ __forceinline__ void butterfly(u64 (&x)[R], int n, const Layout &y) {
    const int low = n < 6 ? n : 6;
    for (int it = 0; it < low; ++it) {
        const u64 m = stage_mask(it);
#pragma unroll
        for (int r = 0; r < R; ++r) x[r] ^= (x[r] >> (1 << it)) & m;
    }
    for (int j = 0; j < y.wl_log; ++j) {           // word-index bits that are lane bits
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const u64 o = shfl_xor64(x[r], 1 << j);
            if (!((y.wl >> j) & 1)) x[r] ^= o;
        }
    }
#pragma unroll
    for (int jr = 0; (1 << jr) < R; ++jr)          // ... and those that are register bits (R > 1: the codeword fills the wave)
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (!((r >> jr) & 1)) x[r] ^= x[r | (1 << jr)];
}

// x = the input bytes of the wave's codewords at their positions: word (codeword gg, index w) is one ballot over the 64 positions
template <int R>
__device__ __forceinline__ void pack(u64 (&x)[R], const PolarSysParams &p, const Layout &y, long base, int lane) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        x[r] = 0;
        for (int s = 0; s < 64; ++s) {
            const long cw = base + (s >> y.wl_log);                       // (wave-uniform)
            if (cw >= p.B) break;
            const int pos = ((r << 6) + (s & (y.WL - 1))) * 64 + lane;
            const unsigned idx = pos < p.N ? p.inv_in[pos] : 0xFFFFu;
            const unsigned bit = idx != 0xFFFFu ? (unsigned)p.in[(size_t)cw * p.K + idx] & 1u : 0u;
            const u64 word = __ballot(bit);
            if (lane == s) x[r] = word;
        }
    }
}

// bit r of the result = parity of rows[r] AND the codeword, the same in all of its lanes
template <int R>
__device__ __forceinline__ unsigned row_parities(const u64 (&x)[R], const uint64_t *rows, int crc, const Layout &y) {
    unsigned pv = 0;
    for (int r = 0; r < crc; ++r) {
        unsigned c = 0;
#pragma unroll
        for (int k = 0; k < R; ++k) c += (unsigned)__popcll(rows[(size_t)r * y.W + (k << 6) + y.wl] & x[k]);
        pv |= (c & 1u) << r;
    }
    for (int off = 1; off < y.WL; off <<= 1) pv ^= (unsigned)__shfl_xor((int)pv, off, 64);
    return pv;
}

// out[cw][i] = bit tab[i] of the codeword (REV: bit bitrev(i)), i < count, for the wave's codewords
template <int R, bool REV>
__device__ __forceinline__ void unpack(const u64 (&x)[R], const PolarSysParams &p, const Layout &y, long base, int lane,
                                       const uint16_t *tab, int count, uint8_t *out) {
    for (int gg = 0; gg < y.G; ++gg) {
        const long cw = base + gg;
        if (cw >= p.B) break;
        for (int i0 = 0; i0 < count; i0 += 64) {
            const int i = i0 + lane;
            const bool on = i < count;
            const unsigned pos = REV ? (__brev((unsigned)(on ? i : 0)) >> (32 - p.n)) : (unsigned)(on ? tab[i] : 0);
            const int w = (int)(pos >> 6);
            u64 v = 0;
#pragma unroll
            for (int k = 0; k < R; ++k) {                                   // (all lanes shuffle, whatever `on`)
                const u64 t = shfl64(x[k], (gg << y.wl_log) + (w & (y.WL - 1)));
                if ((w >> y.wl_log) == k) v = t;
            }
            if (on) out[(size_t)cw * count + i] = (uint8_t)((v >> (pos & 63u)) & 1u);
        }
    }
}

template <int R>
__global__ __launch_bounds__(64) void sys_precode_kernel(PolarSysParams p) {
    const int lane = threadIdx.x;
    const Layout y = make_layout<R>(p.N, lane);
    u64 mask[R];
#pragma unroll
    for (int k = 0; k < R; ++k) mask[k] = p.mask[(k << 6) + y.wl];
    for (long base = (long)blockIdx.x * y.G; base < p.B; base += (long)gridDim.x * y.G) {
        u64 x0[R], u[R], t[R];
        pack<R>(x0, p, y, base, lane);
#pragma unroll
        for (int k = 0; k < R; ++k) u[k] = x0[k];
        for (int d = 0; d < p.depth; ++d) {
#pragma unroll
            for (int k = 0; k < R; ++k) t[k] = u[k];
            butterfly<R>(t, p.n, y);
#pragma unroll
            for (int k = 0; k < R; ++k) u[k] = x0[k] ^ u[k] ^ (t[k] & mask[k]);
        }
        if (p.crc > 0) {
            const unsigned s = row_parities<R>(u, p.rows, p.crc, y);
            for (int r = 0; r < p.crc; ++r)
                if (__popc(p.qinv[r] & s) & 1) {
#pragma unroll
                    for (int k = 0; k < R; ++k) u[k] ^= p.dv[(size_t)r * y.W + (k << 6) + y.wl];
                }
        }
        if (p.out) unpack<R, false>(u, p, y, base, lane, p.gather, p.K, p.out);
        if (p.coded) {
            butterfly<R>(u, p.n, y);
            unpack<R, true>(u, p, y, base, lane, nullptr, p.N, p.coded);
        }
    }
}

template <int R>
__global__ __launch_bounds__(64) void sys_message_kernel(PolarSysParams p) {
    const int lane = threadIdx.x;
    const Layout y = make_layout<R>(p.N, lane);
    for (long base = (long)blockIdx.x * y.G; base < p.B; base += (long)gridDim.x * y.G) {
        u64 u[R];
        pack<R>(u, p, y, base, lane);
        if (p.crc > 0) {                            // the check bits the CRC matrix gives (their positions are empty after the pack)
            const unsigned pv = row_parities<R>(u, p.rows, p.crc, y);
            for (int r = 0; r < p.crc; ++r) {
                const unsigned pos = p.chk[r];
                const int w = (int)(pos >> 6);
#pragma unroll
                for (int k = 0; k < R; ++k)
                    if ((w >> y.wl_log) == k && (w & (y.WL - 1)) == y.wl) u[k] |= (u64)((pv >> r) & 1u) << (pos & 63u);
            }
        }
        butterfly<R>(u, p.n, y);
        unpack<R, false>(u, p, y, base, lane, p.gather, p.K, p.out);
    }
}

// ---- soft message outputs: one lane per (row, message bit) ----
__global__ __launch_bounds__(256) void sys_soft_kernel(const void *llr, int fmt, const double *ext, const uint16_t *pos, long B, int N,
                                                        int K, double *msg_llr) {
    const long total = B * (long)K;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long b = e / K;
        const size_t src = (size_t)b * (size_t)N + pos[e - b * K];
        const double l = fmt ? llr_load_narrow(llr, src, fmt) : reinterpret_cast<const double *>(llr)[src];
        msg_llr[e] = l + ext[src];
    }
}

// ---- the systematic workload around the precode ----
// the info bits of synth_kernel's trials (polar_channel.hip: the same generator calls)
__global__ __launch_bounds__(64) void sys_draw_kernel(PolarEncodeParams p) {
    const int lane = threadIdx.x;
    for (long b = blockIdx.x; b < p.B; b += gridDim.x) {
        const uint64_t trial = p.trial0 + (uint64_t)b * (uint64_t)p.stride;
        const uint64_t block = trial / (uint64_t)p.info_block_div;
        for (int i = lane; i < p.K; i += 64) {
            uint32_t r[4];
            polar_synth_info_word(p.seed, block, (uint32_t)(i >> 7), r);
            const int k = i & 127;
            p.info_out[(size_t)b * p.K + i] = (uint8_t)((r[(k >> 5) & 3] >> (k & 31)) & 1u);
        }
    }
}
// synth_kernel's channel over given coded bits
__global__ __launch_bounds__(64) void sys_channel_kernel(PolarEncodeParams p, const uint8_t *coded) {
    const int lane = threadIdx.x;
    for (long b = blockIdx.x; b < p.B; b += gridDim.x) {
        const uint64_t trial = p.trial0 + (uint64_t)b * (uint64_t)p.stride;
        const uint8_t *c = coded + (size_t)b * p.N;
        if (p.constellation != 0) {
            const int nb = polar_const_nbits(p.constellation);
            const int nsym = p.N / nb;
            double *dl = p.llr + (size_t)b * p.N;
            for (int i = nsym * nb + lane; i < p.N; i += 64) dl[i] = 0.0;
            for (int i = lane; i < nsym; i += 64) {
                int sym = 0;
                for (int j = 0; j < nb; ++j) sym += (1 << j) * (int)c[i * nb + j];
                const double x = polar_const_point(p.constellation, sym) / p.cnorm;
                const double yv = x + polar_synth_symbol_noise(p.seed, trial, (uint32_t)i) * p.sigma;
                double l4[4];
                polar_synth_bicm_demap(p.constellation, p.cnorm, yv, p.n0, l4);
                for (int j = 0; j < nb; ++j) dl[(size_t)i * nb + j] = l4[j];
            }
            continue;
        }
        double2 *dst = reinterpret_cast<double2 *>(p.llr + (size_t)b * p.N);
        for (int pr = lane; pr < p.N / 2; pr += 64) {
            double z0, z1;
            polar_synth_noise_pair(p.seed, trial, (uint32_t)pr, &z0, &z1);
            const int c0 = c[2 * pr], c1 = c[2 * pr + 1];
            double2 v;
            v.x = polar_synth_llr(p.s, c0, z0);
            v.y = polar_synth_llr(p.s, c1, z1);
            dst[pr] = v;
        }
    }
}

// The counters of the sweep (polar_mc_batch_sys): one wave per codeword. ctr[POLAR_SY_*]: runs, block errors (the u-domain words
// differ), wrong message bits, wrong u-domain info bits. A wave counts in registers and adds once per class.
__global__ __launch_bounds__(64) void sys_classify_kernel(const uint8_t *u_dec, const uint8_t *u_sent, const uint8_t *m_dec,
                                                           const uint8_t *m_sent, long B, int K, unsigned long long *ctr) {
    const int lane = threadIdx.x;
    unsigned long long cnt[4] = {0, 0, 0, 0};
    for (long c = blockIdx.x; c < B; c += gridDim.x) {
        const size_t o = (size_t)c * K;
        unsigned du = 0, dm = 0;
        for (int i = lane; i < K; i += 64) {
            du += (u_dec[o + i] != u_sent[o + i]) ? 1u : 0u;
            dm += (m_dec[o + i] != m_sent[o + i]) ? 1u : 0u;
        }
        for (int off = 32; off >= 1; off >>= 1) {
            du += (unsigned)__shfl_xor((int)du, off, 64);
            dm += (unsigned)__shfl_xor((int)dm, off, 64);
        }
        cnt[0] += 1; cnt[1] += du != 0; cnt[2] += dm; cnt[3] += du;
    }
    if (lane == 0)
        for (int k = 0; k < 4; ++k)
            if (cnt[k]) atomicAdd(ctr + k, cnt[k]);
}

int sys_grid(const PolarSysParams &p) {
    const int W = p.N >= 64 ? p.N / 64 : 1;
    const long G = W >= 64 ? 1 : 64 / W;
    const long waves = (p.B + G - 1) / G;
    return (int)(waves < kGridCap ? (waves > 0 ? waves : 1) : kGridCap);
}

}  // namespace

#define SYS_DISPATCH(kernel)                                                                    \
    switch (p.N >> 12) {                                                                        \
        case 0: case 1: hipLaunchKernelGGL(kernel<1>, dim3(sys_grid(p)), dim3(64), 0, st, p); break; \
        case 2: hipLaunchKernelGGL(kernel<2>, dim3(sys_grid(p)), dim3(64), 0, st, p); break;    \
        case 4: hipLaunchKernelGGL(kernel<4>, dim3(sys_grid(p)), dim3(64), 0, st, p); break;    \
        case 8: hipLaunchKernelGGL(kernel<8>, dim3(sys_grid(p)), dim3(64), 0, st, p); break;    \
        default: return hipErrorInvalidValue;                                                   \
    }

hipError_t polar_launch_sys_precode(const PolarSysParams &p, hipStream_t st) {
    if (p.n < 1 || p.N != (1 << p.n) || !p.in || (!p.out && !p.coded)) return hipErrorInvalidValue;
    if (p.B <= 0) return hipSuccess;
    SYS_DISPATCH(sys_precode_kernel)
    return hipGetLastError();
}
hipError_t polar_launch_sys_message(const PolarSysParams &p, hipStream_t st) {
    if (p.n < 1 || p.N != (1 << p.n) || !p.in || !p.out) return hipErrorInvalidValue;
    if (p.B <= 0) return hipSuccess;
    SYS_DISPATCH(sys_message_kernel)
    return hipGetLastError();
}
hipError_t polar_launch_sys_soft(const void *llr, int llr_fmt, const double *ext, const uint16_t *pos, long B, int N, int K,
                                 double *msg_llr, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    const long blocks = (B * (long)K + 255) / 256;
    hipLaunchKernelGGL(sys_soft_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, llr, llr_fmt, ext, pos, B, N, K,
                       msg_llr);
    return hipGetLastError();
}
hipError_t polar_launch_sys_draw(const PolarEncodeParams &p, hipStream_t st) {
    if (p.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(sys_draw_kernel, dim3(polar_rows_grid(p.B)), dim3(64), 0, st, p);
    return hipGetLastError();
}
hipError_t polar_launch_sys_channel(const PolarEncodeParams &p, const uint8_t *coded, hipStream_t st) {
    if (p.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(sys_channel_kernel, dim3(polar_rows_grid(p.B)), dim3(64), 0, st, p, coded);
    return hipGetLastError();
}
hipError_t polar_launch_sys_classify(const uint8_t *u_dec, const uint8_t *u_sent, const uint8_t *m_dec, const uint8_t *m_sent, long B,
                                     int K, unsigned long long *ctr, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(sys_classify_kernel, dim3(polar_rows_grid(B)), dim3(64), 0, st, u_dec, u_sent, m_dec, m_sent, B, K, ctr);
    return hipGetLastError();
}
