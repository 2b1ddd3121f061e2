// polar_kernels_metric.hip — the path metric of a GIVEN word (polar_path_metric_batch*): successive cancellation along
// decisions that are all known in advance, so nothing in it is sequential except the sum at the end.
//
// One wave per (codeword, word). (1) The decision vector u — the word's K info bits, the check bits the handle's CRC matrix gives
// for them, frozen bits 0 — and from it the partial sums of ALL n layers: they are the intermediate stages of the polar transform
// of u, n butterfly stages on bit-packed words in LDS. (2) The LLR pass: n stages of N/2 independent (f, g) pairs, in place — a
// pair's two results take its two input slots, which puts element j of node v of layer lam at address (j << lam) | bitrev_lam(v);
// the partial sums are kept in the same addressing. (3) The N leaf terms log(1 + e^-+llr), in place, then ONE fp64 chain over them in
// leaf order: the list kernels add per leaf in order (prefix_kernel, the rate-0 blocks, the leaf step), and only the same chain
// gives the same bits (tests/test_gpu_list_stats.py compares them as 64-bit patterns).
//
// Beside it list_classify_kernel, the counters of the list statistics (polar_mc_batch_list): it lives here and not next to
// list_find_kernel because polar_channel.hip's existing kernels keep their machine code only while that unit stays as it is.
//
// Arithmetic: polar_llr_nodes.h, the LLR-domain list kernel's own — f_node, g_node, leaf_terms<false>. Built with the common flags;
// -ffp-contract=off is what keeps the operations those of the list kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "polar_kernels.h"
#include "polar_device.h"
#include "polar_edom.h"
#include "polar_llr_nodes.h"
#include "polar_wave_frame.h"

namespace {

// INLDS: the N doubles of the pass live in LDS (behind the tables; the word's info bytes are staged in the same place before the
// channel row is read); else in the block's slice of p.scr, and the info bytes behind the partial sums.
template <bool INLDS>
__global__ __launch_bounds__(64) void path_metric_kernel(PolarMetricParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *tabs = reinterpret_cast<double *>(smem);                              // T[64] RC[129] LC[129] (+2 pad)
    const int n = p.n, N = p.N, K = p.K, NW = packed_words(N);
    double *D = INLDS ? reinterpret_cast<double *>(smem + 324 * 8) : p.scr + (size_t)blockIdx.x * (size_t)N;
    uint32_t *P = reinterpret_cast<uint32_t *>(smem + 324 * 8 + (INLDS ? (size_t)N * 8 : 0));    // [n][NW]: layer lam at (lam - 1) NW
    uint8_t *inf = INLDS ? reinterpret_cast<uint8_t *>(smem + 324 * 8) : reinterpret_cast<uint8_t *>(P + (size_t)n * NW);
    const int lane = threadIdx.x;
    for (int i = lane; i < 322; i += 64) tabs[i] = p.tabs[i];
    const Tabs tb = {tabs, tabs + 64, tabs + 64 + 129};
    const long W = p.B * (long)p.R;
    uint32_t *Pn = P + (size_t)(n - 1) * NW;                                      // the leaves: bit A = u[bitrev_n(A)]
    for (long w = blockIdx.x; w < W; w += gridDim.x) {
        const long b = w / p.R;
        // ---- (1) decisions and partial sums ----
        const uint8_t *info = p.info + (size_t)w * (size_t)K;
        for (int i = lane; i < K; i += 64) inf[i] = info[i];
        for (int i = lane; i < NW; i += 64) Pn[i] = 0u;
        wave_mem_fence();
        for (int i = lane; i < K; i += 64) {
            if (inf[i] & 1u) {
                const unsigned a = __brev((unsigned)p.order[i]) >> (32 - n);
                atomicOr(&Pn[a >> 5], 1u << (a & 31));
            }
        }
        for (int r = 0; r < p.crc; ++r) {                                          // PolarCode.cpp:78-85
            unsigned par = 0;
            for (int j = lane; j < K; j += 64) par ^= (unsigned)(p.crcm[(size_t)r * K + j] & inf[j]);
            const u64 m = __ballot(par & 1u);
            if (lane == 0 && (__popcll(m) & 1)) {
                const unsigned a = __brev((unsigned)p.order[K + r]) >> (32 - n);
                atomicOr(&Pn[a >> 5], 1u << (a & 31));
            }
        }
        wave_mem_fence();
        // layer lam - 1 from layer lam: x[A] ^= x[A + h] where bit h of A is clear, h = 2^(lam - 1)
        for (int lam = n; lam >= 2; --lam) {
            const int h = 1 << (lam - 1);
            const uint32_t *src = P + (size_t)(lam - 1) * NW;
            uint32_t *dst = P + (size_t)(lam - 2) * NW;
            if (h < 32) {
                const uint32_t mask = h == 1 ? 0x55555555u : h == 2 ? 0x33333333u : h == 4 ? 0x0F0F0F0Fu : h == 8 ? 0x00FF00FFu : 0x0000FFFFu;
                for (int i = lane; i < NW; i += 64) { const uint32_t x = src[i]; dst[i] = x ^ ((x >> h) & mask); }
            } else {
                const int hw = h >> 5;
                for (int i = lane; i < NW; i += 64) dst[i] = (i & hw) ? src[i] : (src[i] ^ src[i + hw]);
            }
            wave_mem_fence();
        }
        // ---- (2) LLR pass: the pair (A, A + h) of layer lam - 1 -> f at A, g at A + h with the left child's partial sum ----
        {
            const size_t row = (size_t)b * (size_t)N;                              // stage 1 reads the channel row (widened in the load)
            const uint32_t *Pl = P;
            for (int q = lane; q < N / 2; q += 64) {
                const double a = p.llr_fmt ? llr_load_narrow(p.llr, row + 2 * q, p.llr_fmt) : reinterpret_cast<const double *>(p.llr)[row + 2 * q];
                const double c = p.llr_fmt ? llr_load_narrow(p.llr, row + 2 * q + 1, p.llr_fmt) : reinterpret_cast<const double *>(p.llr)[row + 2 * q + 1];
                const int A = 2 * q;
                const unsigned u = get_bit(Pl, A);
                D[A] = f_node(a, c, tb);
                D[A + 1] = g_node(a, c, u);
            }
            wave_mem_fence();
        }
        for (int lam = 2; lam <= n; ++lam) {
            const int h = 1 << (lam - 1);
            const uint32_t *Pl = P + (size_t)(lam - 1) * NW;
            for (int q = lane; q < N / 2; q += 64) {
                const int A = ((q >> (lam - 1)) << lam) | (q & (h - 1));
                const double a = D[A], c = D[A + h];
                const unsigned u = get_bit(Pl, A);
                D[A] = f_node(a, c, tb);
                D[A + h] = g_node(a, c, u);
            }
            wave_mem_fence();
        }
        // ---- (3) leaf terms in place (address A holds leaf bitrev_n(A)), then the sum in leaf order ----
        for (int A = lane; A < N; A += 64) {
            bool ng; double al, sneg, spos;
            leaf_terms<false>(D[A], true, 0ull, tb, ng, al, sneg, spos);
            const bool one = get_bit(Pn, A) != 0;
            D[A] = (ng != one) ? spos : sneg;                                      // decision 0: log(1 + e^-llr); 1: log(1 + e^llr)
        }
        wave_mem_fence();
        double acc = 0.0;
#pragma unroll 8
        for (int v = 0; v < N; ++v) acc = acc + D[__brev((unsigned)v) >> (32 - n)];
        if (lane == 0) p.pm[w] = acc;
        wave_mem_fence();
    }
}

// list statistics (polar_mc_batch_list): one wave per codeword classifies its list output against the sent word.
// ctr[0] runs, [1] block errors (cand[winner] != sent; K zeros for winner -1), [2] list misses (no row < n_active holds the sent
// info), [3] undetected errors (an error whose winner passed the CRC), [4] of those the ones whose winner is at least as likely as
// the sent word (pm[winner] <= pm_sent): an ML decoder errs too. A wave counts its codewords in registers and adds once per class.
__global__ __launch_bounds__(64) void list_classify_kernel(const uint8_t *cand, const double *pm, const uint8_t *crc_ok,
                                                            const int32_t *n_active, const int32_t *winner, const uint8_t *sent,
                                                            const double *pm_sent, long B, int L, int K, const unsigned int *n_dev,
                                                            unsigned long long *ctr) {
    const int lane = threadIdx.x;
    if (n_dev && (long)*n_dev < B) B = (long)*n_dev;
    unsigned long long cnt[5] = {0, 0, 0, 0, 0};
    for (long c = blockIdx.x; c < B; c += gridDim.x) {
        int na = n_active[c];
        na = na < 0 ? 0 : (na > L ? L : na);
        const int win = winner[c];
        const bool has = win >= 0 && win < L;
        const uint8_t *want = sent + (size_t)c * K;
        const uint8_t *wrow = cand + ((size_t)c * L + (has ? win : 0)) * (size_t)K;
        bool diff = false;
        for (int i = lane; i < K; i += 64) diff |= ((has ? wrow[i] : (uint8_t)0) != want[i]);
        const bool err = __ballot(diff) != 0;
        bool found = false;
        for (int r = 0; r < na && !found; ++r) {
            const uint8_t *row = cand + ((size_t)c * L + r) * (size_t)K;
            bool d = false;
            for (int i = lane; i < K; i += 64) d |= (row[i] != want[i]);
            found = __ballot(d) == 0;                                 // (wave-uniform; rows_differ would change this kernel's machine code)
        }
        const bool undet = err && has && crc_ok[(size_t)c * L + win] == 1;
        const bool ml = undet && pm[(size_t)c * L + win] <= pm_sent[c];
        cnt[0] += 1; cnt[1] += err; cnt[2] += !found; cnt[3] += undet; cnt[4] += ml;
    }
    if (lane == 0)
        for (int k = 0; k < 5; ++k)
            if (cnt[k]) atomicAdd(ctr + k, cnt[k]);
}

}  // namespace

size_t polar_metric_lds_bytes(int n, int in_lds) {
    const int N = 1 << n;
    const size_t sums = (size_t)n * packed_words(N) * 4;
    return 324 * 8 + (in_lds ? (size_t)N * 8 + sums : sums + (size_t)N);          // (K <= N info bytes behind the sums)
}
hipError_t polar_launch_path_metric(const PolarMetricParams &p, int grid, hipStream_t st) {
    const int in_lds = p.scr == nullptr;
    const size_t lds = polar_metric_lds_bytes(p.n, in_lds);
    const void *fn = in_lds ? reinterpret_cast<const void *>(path_metric_kernel<true>) : reinterpret_cast<const void *>(path_metric_kernel<false>);
    if (hipError_t e = polar_allow_lds(fn, lds)) return e;
    if (in_lds) hipLaunchKernelGGL(path_metric_kernel<true>, dim3(grid), dim3(64), lds, st, p);
    else hipLaunchKernelGGL(path_metric_kernel<false>, dim3(grid), dim3(64), lds, st, p);
    return hipGetLastError();
}
hipError_t polar_launch_list_classify(const uint8_t *cand, const double *pm, const uint8_t *crc_ok, const int32_t *n_active,
                                      const int32_t *winner, const uint8_t *sent, const double *pm_sent, long B, int L, int K,
                                      const unsigned int *n_dev, unsigned long long *ctr, hipStream_t st) {
    hipLaunchKernelGGL(list_classify_kernel, dim3(polar_rows_grid(B)), dim3(64), 0, st, cand, pm, crc_ok, n_active, winner, sent, pm_sent, B, L, K,
                       n_dev, ctr);
    return hipGetLastError();
}
