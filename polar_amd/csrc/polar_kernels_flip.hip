// polar_kernels_flip.hip — SC-Flip (polar_decode_sc_flip_batch*): plain successive cancellation in the LLR domain, and
// while the word fails the CRC, whole re-decodes with ONE decision inverted — the unfrozen leaves of smallest |LLR| of the first pass,
// least reliable first (Afisiadis, Balatsoukas-Stimming, Burg 2014).
//
// One codeword per wave, grid-stride over the rows. LDS: the 322 table doubles, then the channel row and every layer below it — layer
// lam holds the N >> lam values of the node the walk is in, 2 N - 1 doubles in all —, then three bit-packed arrays of N bits: the
// partial sums X, the decisions U of the pass, the decisions U0 of pass 0. The row is read from HBM once and stays for every retry.
//
// The walk is a schedule the host builds once per handle (polar_flip.cpp flip_schedule): F and G steps into a child, QUAD for a node
// of four leaves (decided in registers), COMBINE once both children of a larger node are done. All-frozen subtrees have no ops at all: their decisions and partial
// sums are zero, and X is zeroed at the start of a pass. Every unfrozen leaf gets its exact LLR — no rate-1 shortcut: the magnitudes
// are the product.
//
// X is ONE array for all layers, in the addressing of path_metric_kernel: element j of node v of layer lam is bit
// (j << lam) | bitrev_lam(v). A node's children interleave into it, so "parent[2j] = left[j] ^ right[j], parent[2j+1] = right[j]" is
// x[A] ^= x[A + h] in place, h = 2^(lam - 1), over the addresses of the parent.
//
// Pass 0 keeps the T smallest (|LLR|, position) of its unfrozen leaves across the lanes, sorted, lane t = rank t; a leaf enters only
// if the list is not full or it is smaller than the largest entry (one wave-uniform compare). Equal magnitudes stay in position order.
//
// Arithmetic: polar_llr_nodes.h — f_node, g_node, the reference's operation order. Built with the common flags (-ffp-contract=off).
// Outputs leave through plain vector stores; the counters of the sweep through atomicAdd.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "polar_kernels.h"
#include "polar_device.h"
#include "polar_edom.h"
#include "polar_llr_nodes.h"
#include "polar_wave_frame.h"

namespace {

__global__ __launch_bounds__(64) void sc_flip_kernel(PolarFlipParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *tabs = reinterpret_cast<double *>(smem);                              // T[64] RC[129] LC[129] (+2 pad)
    const int n = p.n, N = p.N, K = p.K, T = p.T, NW = packed_words(N);
    double *lay = reinterpret_cast<double *>(smem + 324 * 8);
    uint32_t *X = reinterpret_cast<uint32_t *>(smem + 324 * 8 + (size_t)2 * N * 8), *U = X + NW, *U0 = U + NW;
    const int lane = threadIdx.x;
    for (int i = lane; i < 322; i += 64) tabs[i] = p.tabs[i];
    const Tabs tb = {tabs, tabs + 64, tabs + 64 + 129};
    const int unfrozen = K + p.crc, T_eff = T < unfrozen ? T : unfrozen;
    const int leaf_at = layer_off(N, n);
    for (long b = blockIdx.x; b < p.B; b += gridDim.x) {
        const size_t row = (size_t)b * (size_t)N;
        for (int i = lane; i < N; i += 64)
            lay[i] = p.llr_fmt ? llr_load_narrow(p.llr, row + i, p.llr_fmt) : reinterpret_cast<const double *>(p.llr)[row + i];
        double my_m = __builtin_inf();                 // rank `lane` of the running T smallest: magnitude, position (-1: empty)
        int my_p = -1, held = 0;
        double cur_max = __builtin_inf();
        int n_dec = T_eff + 1, flip = -1;
        bool ok = false;
        for (int att = 0; att <= T_eff && !ok; ++att) {
            const int c = att ? __shfl(my_p, att - 1, 64) : -1;
            for (int i = lane; i < NW; i += 64) { X[i] = 0u; U[i] = 0u; }
            wave_mem_fence();
            // A node of two leaves in registers, every lane the same values: f and the left decision, g and the right one. fz: bit
            // `side` set = that leaf is frozen and decides 0 unseen. Returns u0 | u1 << 1.
            auto pair = [&](double a, double c2, int phi0, int fz) -> unsigned {
                unsigned u[2] = {0u, 0u};
                for (int side = 0; side < 2; ++side) {
                    if ((fz >> side) & 1) continue;                               // (wave-uniform)
                    const int phi = phi0 + side;
                    const double v = readlane_d(side ? g_node(a, c2, u[0]) : f_node(a, c2, tb), 0);
                    u[side] = (unsigned)(v < 0) ^ (unsigned)(phi == c);
                    if (lane == 0 && u[side]) U[phi >> 5] |= 1u << (phi & 31);
                    const double m = fabs(v);
                    if (att == 0 && T > 0 && (held < T || m < cur_max)) {         // (wave-uniform)
                        const double pm = __shfl_up(my_m, 1, 64);
                        const int pp = __shfl_up(my_p, 1, 64);
                        const bool stays = my_p >= 0 && my_m <= m;                // equal magnitudes: the earlier position first
                        const bool before = lane == 0 || (pp >= 0 && pm <= m);
                        if (lane < T && !stays) {
                            my_m = before ? m : pm;
                            my_p = before ? phi : pp;
                        }
                        held = held < T ? held + 1 : T;
                        cur_max = readlane_d(my_m, T - 1);
                    }
                }
                return u[0] | (u[1] << 1);
            };
            auto set_x = [&](int A, unsigned bit) { if (bit) X[A >> 5] |= 1u << (A & 31); };      // (lane 0; X is zero where not yet written)
            for (int base = 0; base < p.n_ops; base += 64) {
                const uint32_t opv = base + lane < p.n_ops ? p.ops[base + lane] : 0u;
                const int cnt = p.n_ops - base < 64 ? p.n_ops - base : 64;
                for (int k = 0; k < cnt; ++k) {
                    const uint32_t op = (uint32_t)__builtin_amdgcn_readlane((int)opv, k);
                    const int type = (int)(op & 7u), lam = (int)((op >> 3) & 15u), arg = (int)(op >> 8);
                    if (type == POLAR_FLIP_OP_F) {
                        const double *par = lay + layer_off(N, lam - 1);
                        double *ch = lay + layer_off(N, lam);
                        for (int j = lane; j < (N >> lam); j += 64) ch[j] = f_node(par[2 * j], par[2 * j + 1], tb);
                    } else if (type == POLAR_FLIP_OP_G) {                        // arg: the address residue of the left sibling
                        const double *par = lay + layer_off(N, lam - 1);
                        double *ch = lay + layer_off(N, lam);
                        for (int j = lane; j < (N >> lam); j += 64) ch[j] = g_node(par[2 * j], par[2 * j + 1], get_bit(X, (j << lam) | arg));
                    } else if (type == POLAR_FLIP_OP_QUAD) {                     // arg: the first leaf's position | frozen flags << 16
                        // a node of four leaves in registers: the two f-nodes of its left child at once (f_node2: their chains
                        // overlap), that pair, the two g-nodes, the right pair, and the node's partial sums straight into X
                        const int phi0 = arg & 0xFFFF, fz = arg >> 16;
                        const double *par = lay + leaf_at - 6;
                        const double a0 = par[0], a1 = par[1], a2 = par[2], a3 = par[3];
                        unsigned ul = 0, ur = 0;
                        if ((fz & 3) != 3) {
                            double l0, l1;
                            f_node2(a0, a1, a2, a3, tb, l0, l1);
                            ul = pair(l0, l1, phi0, fz & 3);
                        }
                        const unsigned xl0 = (ul ^ (ul >> 1)) & 1u, xl1 = ul >> 1;
                        if ((fz >> 2) != 3) ur = pair(g_node(a0, a1, xl0), g_node(a2, a3, xl1), phi0 + 2, fz >> 2);
                        const unsigned xr0 = (ur ^ (ur >> 1)) & 1u, xr1 = ur >> 1;
                        if (lane == 0) {
                            const int A0 = (int)(__brev((unsigned)phi0) >> (32 - n)), q = N >> 2;
                            set_x(A0, xl0 ^ xr0); set_x(A0 + q, xr0); set_x(A0 + 2 * q, xl1 ^ xr1); set_x(A0 + 3 * q, xr1);
                        }
                    } else if (type == POLAR_FLIP_OP_PAIR) {                     // (n = 1 only: the root) arg as QUAD's
                        const unsigned u = pair(lay[0], lay[1], arg & 0xFFFF, arg >> 16);
                        if (lane == 0) { set_x(0, (u ^ (u >> 1)) & 1u); set_x(1, u >> 1); }
                    } else {                                                     // COMBINE into the parent; lam: the children's layer,
                        const int h = 1 << (lam - 1);                            // arg: the parent's address residue (< h)
                        if (lam <= 5) {
                            const uint32_t rep = lam == 1 ? 0x55555555u : lam == 2 ? 0x11111111u : lam == 3 ? 0x01010101u : lam == 4 ? 0x00010001u : 1u;
                            const uint32_t mask = rep << arg;
                            for (int i = lane; i < NW; i += 64) { const uint32_t x = X[i]; X[i] = x ^ ((x >> h) & mask); }
                        } else {
                            const int hw = h >> 5, w0 = arg >> 5;
                            const uint32_t mask = 1u << (arg & 31);
                            for (int j = lane; j < (N >> lam); j += 64) {
                                const int w = (j << (lam - 5)) | w0;
                                X[w] ^= X[w + hw] & mask;
                            }
                        }
                    }
                    wave_mem_fence();
                }
            }
            ok = crc_matches(p, lane, [&](int pos) { return get_bit(U, pos); });
            if (ok) { n_dec = att + 1; flip = c; }
            else if (att == 0) {
                for (int i = lane; i < NW; i += 64) U0[i] = U[i];
                wave_mem_fence();
            }
        }
        const uint32_t *Wd = ok ? U : U0;
        uint8_t *out = p.out + (size_t)b * (size_t)K;
        for (int i = lane; i < K; i += 64) out[i] = (uint8_t)get_bit(Wd, p.order[i]);
        if (lane == 0) {
            if (p.crc_ok) p.crc_ok[b] = ok ? 1 : 0;
            if (p.n_dec) p.n_dec[b] = (uint8_t)n_dec;
            if (p.flip) p.flip[b] = flip;
        }
        if (lane < T) {
            if (p.cand) p.cand[(size_t)b * T + lane] = my_p;
            if (p.mag) p.mag[(size_t)b * T + lane] = my_m;
        }
        wave_mem_fence();
    }
}

// The counters of the sweep (polar_mc_batch_flip): one wave per codeword, the delivered word against the sent one. ctr[POLAR_FL_*]:
// runs, block errors (out != sent), undetected errors (an error delivered with crc_ok = 1), first-pass words (crc_ok = 1, n_dec == 1), words a
// retry delivered (crc_ok = 1, n_dec > 1), the sum of n_dec. A wave counts in registers and adds once per class.
__global__ __launch_bounds__(64) void flip_classify_kernel(const uint8_t *out, const uint8_t *crc_ok, const uint8_t *n_dec,
                                                            const uint8_t *sent, long B, int K, unsigned long long *ctr) {
    const int lane = threadIdx.x;
    unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};
    for (long c = blockIdx.x; c < B; c += gridDim.x) {
        const uint8_t *got = out + (size_t)c * K, *want = sent + (size_t)c * K;
        const bool err = rows_differ(got, want, K, lane);
        const bool ok = crc_ok[c] == 1;
        const unsigned nd = n_dec[c];
        cnt[0] += 1; cnt[1] += err; cnt[2] += (err && ok); cnt[3] += (ok && nd == 1); cnt[4] += (ok && nd > 1); cnt[5] += nd;
    }
    if (lane == 0)
        for (int k = 0; k < 6; ++k)
            if (cnt[k]) atomicAdd(ctr + k, cnt[k]);
}

}  // namespace

size_t polar_flip_lds_bytes(int N) { return 324 * 8 + (size_t)2 * N * 8 + (size_t)3 * packed_words(N) * 4; }
int polar_flip_max_log() { return 12; }            // 16 N bytes of LDS per wave: 64 KiB at N = 4096
int polar_flip_grid_cap() { return 8192; }
hipError_t polar_launch_sc_flip(const PolarFlipParams &p, int grid, hipStream_t st) {
    const size_t lds = polar_flip_lds_bytes(p.N);
    if (hipError_t e = polar_allow_lds(reinterpret_cast<const void *>(sc_flip_kernel), lds)) return e;
    hipLaunchKernelGGL(sc_flip_kernel, dim3(grid), dim3(64), lds, st, p);
    return hipGetLastError();
}
hipError_t polar_launch_flip_classify(const uint8_t *out, const uint8_t *crc_ok, const uint8_t *n_dec, const uint8_t *sent, long B, int K,
                                      unsigned long long *ctr, hipStream_t st) {
    hipLaunchKernelGGL(flip_classify_kernel, dim3(polar_rows_grid(B)), dim3(64), 0, st, out, crc_ok, n_dec, sent,
                       B, K, ctr);
    return hipGetLastError();
}
