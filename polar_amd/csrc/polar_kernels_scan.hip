// polar_kernels_scan.hip — SCAN soft-output decoding (polar_decode_scan_batch*): soft cancellation (Fayyaz, Barry 2014),
// the SC schedule with LLRs passed in both directions and a few iterations. Node v of layer lam has N >> lam values and the children
// 2v (left) and 2v + 1 (right), which pair its neighbouring elements 2j, 2j + 1 as sc_flip_kernel does. Every node carries L (down,
// the channel row at layer 0) and B (up; a leaf's is +inf if frozen, else 0; every internal B is 0 before iteration 1). At a node with
// values a, a0 = a[2j], a1 = a[2j+1], one iteration is
//   L_left[j]  = f(a0, a1 + B_right[j])          (B_right: the previous iteration's)
//   L_right[j] = f(a0, B_left[j]) + a1
//   B[2j]      = f(B_left[j], B_right[j] + a1),  B[2j+1] = f(B_left[j], a0) + B_right[j]
// depth first. f is f_node (polar_llr_nodes.h) or, under POLAR_SCAN_MINSUM, sgn sgn min with +0 where the min is 0.
//
// One codeword per wave, grid-stride over the rows. LDS, in doubles: the 322 table doubles (+2 pad); L: the row and every layer below
// it, layer lam holding the node the walk is in (2 N); the B of the LEFT child that is open per layer (N; transient: it is consumed by
// the sibling's L and the parent's B before the walk opens another node of that layer); the B of every RIGHT child of layers 1 .. n-1
// ((n - 1) N / 2; it persists into the next iteration and is zeroed per row); the leaf LLRs in decoding order (N). 150 048 bytes at
// n = 11: one wave per CU.
//
// The walk is a schedule the host builds once per handle (polar_scan.cpp scan_schedule): LEFT and RIGHT steps into a child, UP once
// both children of a node are done, PAIR for a node of two leaves (in registers: both leaf LLRs and the node's B). An all-frozen
// subtree has B = +inf everywhere and an all-unfrozen one B = 0: neither is computed or stored, the steps that would read them take
// the constant instead — the SAME expressions on it, so pruning changes no value. (The one step that reads a B of the PREVIOUS
// iteration, LEFT, takes 0 for an all-frozen right sibling in iteration 1: internal B start at 0. No construction freezes a right
// child whose left sibling is not frozen, an explicit frozen set may.) Nothing walks into an all-frozen subtree (its leaf LLRs are
// never read); an all-unfrozen one is walked for its leaf LLRs but has no UP steps.
//
// f with a zero argument is +0 under both arithmetics (f_node's value there too: log 1), and is returned before f_node is entered:
// the B = 0 of unfrozen leaves would otherwise send every such element through f_node's libm path for arguments below 1e-6.
// Built with the common flags (-ffp-contract=off). Outputs leave through plain vector stores; the sweep's counters through atomicAdd.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "polar_kernels.h"
#include "polar_device.h"
#include "polar_edom.h"
#include "polar_llr_nodes.h"
#include "polar_wave_frame.h"

namespace {

__host__ __device__ inline size_t scan_lds_doubles(int n, int N) { return 324 + (size_t)4 * N + (size_t)(n - 1) * (N / 2); }

template <bool MS>
__device__ __forceinline__ double scan_f(double a, double b, const Tabs &tb) {
    const double mn = __builtin_fmin(fabs(a), fabs(b));
    if (MS) {
        const int sx = (__double2hiint(a) ^ __double2hiint(b)) & (int)0x80000000;
        const double ms = __hiloint2double(__double2hiint(mn) | sx, __double2loint(mn));
        return mn == 0.0 ? 0.0 : ms;
    } else {
        if (mn == 0.0) return 0.0;
        return f_node(a, b, tb);
    }
}
// the B of a child that is all frozen / all unfrozen
__device__ __forceinline__ double kind_const(int kind) { return kind == POLAR_SCAN_KIND_FROZEN ? __builtin_inf() : 0.0; }

template <bool MS>
__global__ __launch_bounds__(64) void scan_kernel(PolarScanParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *tabs = reinterpret_cast<double *>(smem);                              // T[64] RC[129] LC[129] (+2 pad)
    const int n = p.n, N = p.N, K = p.K, H = N / 2;
    double *lay = tabs + 324;                   // L: layer lam at layer_off(N, lam)
    double *bl = lay + 2 * N;                   // B of the open left child: layer lam (>= 1) at layer_off(N, lam) - N
    double *br = bl + N;                        // B of the right children: layer lam (1 .. n-1) at (lam - 1) H, node 2w + 1 at w (N >> lam)
    double *leaf = br + (size_t)(n - 1) * H;    // leaf LLRs, decoding order
    const int lane = threadIdx.x;
    if (!MS)
        for (int i = lane; i < 322; i += 64) tabs[i] = p.tabs[i];
    const Tabs tb = {tabs, tabs + 64, tabs + 64 + 129};
    const bool early = (p.flags & POLAR_SCAN_F_EARLY) != 0;
    for (long b = blockIdx.x; b < p.B; b += gridDim.x) {
        const size_t row = (size_t)b * (size_t)N;
        for (int i = lane; i < N; i += 64)
            lay[i] = p.llr_fmt ? llr_load_narrow(p.llr, row + i, p.llr_fmt) : reinterpret_cast<const double *>(p.llr)[row + i];
        for (int i = lane; i < (n - 1) * H; i += 64) br[i] = 0.0;
        // (leaf[] needs no reset: every unfrozen leaf is written in each iteration before anything reads it, a frozen one is never read)
        wave_mem_fence();
        double *ext = p.ext ? p.ext + row : nullptr;
        int n_it = 0;
        bool ok = p.crc == 0;
        for (int it = 0; it < p.iters; ++it) {
            for (int base = 0; base < p.n_ops; base += 64) {
                const uint32_t opv = base + lane < p.n_ops ? p.ops[base + lane] : 0u;
                const int cnt = p.n_ops - base < 64 ? p.n_ops - base : 64;
                for (int k = 0; k < cnt; ++k) {
                    const uint32_t op = (uint32_t)__builtin_amdgcn_readlane((int)opv, k);
                    const int type = (int)(op & 7u), lam = (int)((op >> 3) & 15u), v = (int)((op >> 7) & 0xFFFFu);
                    const int kl = (int)((op >> 23) & 3u), kr = (int)((op >> 25) & 3u);
                    if (type == POLAR_SCAN_OP_LEFT) {                           // lam: the child's layer, v: the parent
                        const int m = N >> lam;
                        const double *par = lay + layer_off(N, lam - 1), *bs = br + (size_t)(lam - 1) * H + (size_t)v * m;
                        double *ch = lay + layer_off(N, lam);
                        const bool mix = kr == POLAR_SCAN_KIND_MIXED;
                        const double bc = it ? kind_const(kr) : 0.0;          // (an internal B is 0 before iteration 1, an all-frozen node's too)
                        for (int j = lane; j < m; j += 64) ch[j] = scan_f<MS>(par[2 * j], par[2 * j + 1] + (mix ? bs[j] : bc), tb);
                    } else if (type == POLAR_SCAN_OP_RIGHT) {
                        const int m = N >> lam;
                        const double *par = lay + layer_off(N, lam - 1), *bs = bl + layer_off(N, lam) - N;
                        double *ch = lay + layer_off(N, lam);
                        const bool mix = kl == POLAR_SCAN_KIND_MIXED;
                        const double bc = kind_const(kl);
                        for (int j = lane; j < m; j += 64) ch[j] = scan_f<MS>(par[2 * j], mix ? bs[j] : bc, tb) + par[2 * j + 1];
                    } else if (type == POLAR_SCAN_OP_UP) {                      // lam: the node's layer (<= n - 2), v: the node
                        const int m = N >> (lam + 1);
                        const double *a = lay + layer_off(N, lam), *sl = bl + layer_off(N, lam + 1) - N, *sr = br + (size_t)lam * H + (size_t)v * m;
                        const bool mixl = kl == POLAR_SCAN_KIND_MIXED, mixr = kr == POLAR_SCAN_KIND_MIXED;
                        const double cl = kind_const(kl), cr = kind_const(kr);
                        double *dst = lam == 0 ? ext : (v & 1) ? br + (size_t)(lam - 1) * H + (size_t)(v >> 1) * (2 * m) : bl + layer_off(N, lam) - N;
                        if (dst)
                            for (int j = lane; j < m; j += 64) {
                                const double a0 = a[2 * j], a1 = a[2 * j + 1], Bl = mixl ? sl[j] : cl, Br = mixr ? sr[j] : cr;
                                const double b0 = scan_f<MS>(Bl, Br + a1, tb), b1 = scan_f<MS>(Bl, a0, tb) + Br;
                                dst[2 * j] = b0;
                                dst[2 * j + 1] = b1;
                            }
                    } else {                                                     // PAIR: the node v of layer lam = n - 1; kl, kr: its leaves
                        const double *a = lay + layer_off(N, lam);
                        const double a0 = a[0], a1 = a[1], Bl = kind_const(kl), Br = kind_const(kr);
                        double l0 = 0.0, l1 = 0.0, b0 = 0.0, b1 = 0.0;
                        if (kl != POLAR_SCAN_KIND_FROZEN) l0 = scan_f<MS>(a0, a1 + Br, tb);
                        if (kr != POLAR_SCAN_KIND_FROZEN) l1 = scan_f<MS>(a0, Bl, tb) + a1;
                        double *dst = nullptr;
                        if ((op >> 27) & 1u) {                                   // the node's B is read (a mixed node, or the root)
                            dst = lam == 0 ? ext : (v & 1) ? br + (size_t)(lam - 1) * H + (size_t)(v >> 1) * 2 : bl + layer_off(N, lam) - N;
                            b0 = scan_f<MS>(Bl, Br + a1, tb);
                            b1 = scan_f<MS>(Bl, a0, tb) + Br;
                        }
                        if (lane == 0) {
                            if (kl != POLAR_SCAN_KIND_FROZEN) leaf[2 * v] = l0;
                            if (kr != POLAR_SCAN_KIND_FROZEN) leaf[2 * v + 1] = l1;
                            if (dst) { dst[0] = b0; dst[1] = b1; }
                        }
                    }
                    wave_mem_fence();
                }
            }
            n_it = it + 1;
            if (p.crc > 0 && (early || it == p.iters - 1)) ok = crc_matches(p, lane, [&](int pos) { return leaf[pos] < 0; });
            if (early && ok) break;
        }
        uint8_t *out = p.out + (size_t)b * (size_t)K;
        for (int i = lane; i < K; i += 64) {
            const double l = leaf[p.order[i]];
            out[i] = (uint8_t)(l < 0);
            if (p.info_llr) p.info_llr[(size_t)b * (size_t)K + i] = l;
        }
        if (lane == 0) {
            if (p.crc_ok) p.crc_ok[b] = ok ? 1 : 0;
            if (p.n_iter) p.n_iter[b] = (uint8_t)n_it;
        }
        wave_mem_fence();
    }
}

// The counters of the sweep (polar_mc_batch_scan): one wave per codeword, the decided word against the sent one. ctr[POLAR_SN_*]:
// runs, block errors (out != sent), undetected errors (the code has a CRC, the word passed it and is wrong), the sum of n_iter. A wave
// counts in registers and adds once per class.
__global__ __launch_bounds__(64) void scan_classify_kernel(const uint8_t *out, const uint8_t *crc_ok, const uint8_t *n_iter,
                                                            const uint8_t *sent, long B, int K, int has_crc, unsigned long long *ctr) {
    const int lane = threadIdx.x;
    unsigned long long cnt[4] = {0, 0, 0, 0};
    for (long c = blockIdx.x; c < B; c += gridDim.x) {
        const uint8_t *got = out + (size_t)c * K, *want = sent + (size_t)c * K;
        bool diff = false;                                            // (written out: rows_differ would change this kernel's machine code)
        for (int i = lane; i < K; i += 64) diff |= (got[i] != want[i]);
        const bool err = __ballot(diff) != 0;
        cnt[0] += 1; cnt[1] += err; cnt[2] += (err && has_crc && crc_ok[c] == 1); cnt[3] += n_iter[c];
    }
    if (lane == 0)
        for (int k = 0; k < 4; ++k)
            if (cnt[k]) atomicAdd(ctr + k, cnt[k]);
}

}  // namespace

size_t polar_scan_lds_bytes(int n) { return scan_lds_doubles(n, 1 << n) * 8; }
int polar_scan_max_log() { return 11; }            // (n + 7) N / 2 doubles of LDS per wave: 147 KiB at N = 2048, twice the device's at 4096
int polar_scan_grid_cap() { return 8192; }
hipError_t polar_launch_scan(const PolarScanParams &p, int grid, hipStream_t st) {
    const size_t lds = polar_scan_lds_bytes(p.n);
    const bool ms = (p.flags & POLAR_SCAN_F_MINSUM) != 0;
    const void *fn = ms ? reinterpret_cast<const void *>(scan_kernel<true>) : reinterpret_cast<const void *>(scan_kernel<false>);
    if (hipError_t e = polar_allow_lds(fn, lds)) return e;
    if (ms) hipLaunchKernelGGL(scan_kernel<true>, dim3(grid), dim3(64), lds, st, p);
    else hipLaunchKernelGGL(scan_kernel<false>, dim3(grid), dim3(64), lds, st, p);
    return hipGetLastError();
}
hipError_t polar_launch_scan_classify(const uint8_t *out, const uint8_t *crc_ok, const uint8_t *n_iter, const uint8_t *sent, long B, int K,
                                      int has_crc, unsigned long long *ctr, hipStream_t st) {
    hipLaunchKernelGGL(scan_classify_kernel, dim3(polar_rows_grid(B)), dim3(64), 0, st, out, crc_ok, n_iter, sent,
                       B, K, has_crc, ctr);
    return hipGetLastError();
}
