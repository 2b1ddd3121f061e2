// polar_kernels_ga.hip — Gaussian-approximation (GA) code construction on the device, fp64 throughout:
//   ga_capacity_kernel   the capacity integrals get_bicm_capacity / get_mlc_capacity (Constellation.m:190-286) and
//                        get_bpsk_cap (CapacityHelper/get_bpsk_cap.m), one block per (SNR, bit / layer);
//   ga_phi_kernel        the two tables of GaussianApproximation/initialize_phi.m;
//   ga_polarized_kernel  the Monte-Carlo polarized capacity of get_polarized_capacity (Constellation.m:288-370): one lane
//                        per symbol, histograms privatised in LDS;
//   ga_construct_kernel  calculate_awgn_polarization.m per sub-block, the stable descending sort and the prefix sums of
//                        qfunc(sqrt(c)/sqrt(2)) along it (PolarCode.m:198-255), one block per design point.
// Build with -ffp-contract=off (as every translation unit of the library). Grids, index rules and deviations from the
// reference's MATLAB colon ranges are written down in DESIGN.md §8b and restated in tests/ga_numpy.py.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "polar_kernels.h"
#include "polar_synth.h"

namespace {

constexpr int T = POLAR_GA_THREADS;

// fixed-shape tree over the block's per-thread partial sums (T a power of two)
__device__ double block_sum(double v, double *sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int s = T / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = sh[t] + sh[t + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(T) void ga_capacity_kernel(PolarGaCapParams p) {
    __shared__ double sh[T];
    const int snr = blockIdx.y, bit = blockIdx.x, t = threadIdx.x;
    const PolarGaGrid g = p.grid[snr];
    const double n0 = g.n0, dy = g.dy;
    if (p.kind == 2) {
        // get_bpsk_cap.m: x in {-1, 1}, p_y normalised by sum(p_y) * dy, h = sum -log2(p) p dy, c = h - 0.5 (1 + ln(2 pi n0)) / ln 2
        const double c = sqrt(2 * M_PI * n0);
        double s = 0.0;
        for (long k = t; k < g.P; k += T) {
            const double y = -g.ymax + (double)k * dy;
            const double a = y - (-1.0), b = y - 1.0;
            double py = 0.0;
            py = py + exp(-(a * a) / 2 / n0) / c * 0.5;
            py = py + exp(-(b * b) / 2 / n0) / c * 0.5;
            s = s + py;
        }
        const double norm = block_sum(s, sh) * dy;
        double h = 0.0;
        for (long k = t; k < g.P; k += T) {
            const double y = -g.ymax + (double)k * dy;
            const double a = y - (-1.0), b = y - 1.0;
            double py = 0.0;
            py = py + exp(-(a * a) / 2 / n0) / c * 0.5;
            py = py + exp(-(b * b) / 2 / n0) / c * 0.5;
            py = py / norm;
            if (py > 0) h = h + (-log2(py)) * py * dy;
        }
        h = block_sum(h, sh);
        if (t == 0) p.out[snr] = h - 0.5 * (1 + log(2 * M_PI * n0)) / log(2.0);
        return;
    }
    const int ns = p.ns;
    const double c = sqrt(2 * M_PI * n0);
    double hy = 0.0, hu = 0.0;
    for (long k = t; k < g.P; k += T) {
        const double y = -g.ymax + (double)k * dy;
        if (p.kind == 0) {
            // get_bicm_capacity (Constellation.m:250-286)
            double py = 0.0, pu0 = 0.0, pu1 = 0.0;
            for (int s = 0; s < ns; ++s) {
                const double d = y - p.pt[s];
                const double e = exp(-(d * d) / 2 / n0) / c / ns;
                py = py + e;
                if ((s >> bit) & 1) pu1 = pu1 + e * 2; else pu0 = pu0 + e * 2;
            }
            if (py > 0) hy = hy + log2(py) * py * dy * (-1);
            if (pu0 > 0) hu = hu + 0.5 * log2(pu0) * pu0 * dy * (-1);
            if (pu1 > 0) hu = hu + 0.5 * log2(pu1) * pu1 * dy * (-1);
        } else {
            // get_mlc_capacity (Constellation.m:190-248): sets = values of the label bits below `bit`
            const int sets = 1 << bit;
            for (int q = 0; q < sets; ++q) {
                double py = 0.0, pu0 = 0.0, pu1 = 0.0;
                for (int s = q; s < ns; s += sets) {
                    const double d = y - p.pt[s];
                    const double e = exp(-(d * d) / 2 / n0) / c / ns;
                    py = py + e;
                    if ((s >> bit) & 1) pu1 = pu1 + e * 2; else pu0 = pu0 + e * 2;
                }
                if (py > 0) hy = hy + (-log2(py)) * py * dy;
                if (pu0 > 0) hu = hu + (-log2(pu0)) * pu0 * 0.5 * dy;
                if (pu1 > 0) hu = hu + (-log2(pu1)) * pu1 * 0.5 * dy;
            }
        }
    }
    hy = block_sum(hy, sh);
    hu = block_sum(hu, sh);
    if (t == 0) p.out[(size_t)snr * p.nb + bit] = hy - hu;
}

// initialize_phi.m. Forward: x = k * 0.01, no +0.0001. Inverse: x = k * dx with the +0.0001 form and min(phi, 1); bin
// ceil(-log(phi) / 1e-3) while -log(phi) < 100 + 1e-3, the largest x wins (the reference's last write); -log through the
// fixed-order polar_synth_log, as in the lookup of the construction kernel. MATLAB grows its table by one for a bin of
// 100001 (-log phi in (100, 100.001)), an entry no lookup reads (the lookup clamps at 100): it is not kept.
constexpr int PHI_RUN = 16;                 // consecutive x per lane: one atomic per bin change
__global__ __launch_bounds__(T) void ga_phi_kernel(double *fwd, unsigned long long *inv, double dx, long nx) {
    const long gid = (long)blockIdx.x * T + threadIdx.x;
    if (gid < POLAR_GA_PHI_FWD) {
        const double x = (double)gid * 0.01;
        fwd[gid] = x < 10 ? exp(-0.4527 * pow(x, 0.86) + 0.0218) : sqrt(M_PI / x) * (1 - 1.4286 / x) * exp(-x / 4);
    }
    long cur = -1;
    double best = 0.0;
    for (long k = gid * PHI_RUN; k < nx && k < (gid + 1) * PHI_RUN; ++k) {
        const double x = (double)k * dx;
        double ph = x < 10 ? exp(-0.4527 * pow(x, 0.86) + 0.0218)
                           : sqrt(M_PI / (x + 0.0001)) * (1 - 1.4286 / (x + 0.0001)) * exp(-x / 4);
        ph = ph < 1 ? ph : 1;
        const double mlp = -polar_synth_log(ph);
        if (!(mlp < 100 + 1e-3)) continue;
        const long b = (long)ceil(mlp / 1e-3);
        if (b < 0 || b >= POLAR_GA_PHI_INV) continue;
        if (b != cur) {
            if (cur >= 0) atomicMax(inv + cur, (unsigned long long)__double_as_longlong(best));
            cur = b; best = x;
        } else if (x > best) {
            best = x;
        }
    }
    if (cur >= 0) atomicMax(inv + cur, (unsigned long long)__double_as_longlong(best));
}

// PolarCode.m:951 cnop_llr, :952-954 vnop_llr
__device__ __forceinline__ double cnop_llr(double a, double b) { return 2 * atanh(tanh(a / 2) * tanh(b / 2)); }
__device__ __forceinline__ double vnop_llr(double a, double b) { return a + b; }

// polar_decode_capacity_llr (PolarCode.m:931-945) for N = 2 on (y0, y1) with message bits (i0, i1)
__device__ __forceinline__ void genie2(double y0, double y1, int i0, double *u) {
    u[0] = cnop_llr(y0, y1);
    u[1] = vnop_llr((1 - 2 * i0) * y0, y1);
}

constexpr int POL_SYM_PER_BLOCK = T * 32;

__global__ __launch_bounds__(T) void ga_polarized_kernel(PolarGaPolParams p) {
    __shared__ unsigned int hist[4 * POLAR_GA_BINS * 2];
    const int snr = blockIdx.y, nb = p.nb, t = threadIdx.x;
    const int nbins = nb * POLAR_GA_BINS * 2;
    for (int i = t; i < nbins; i += T) hist[i] = 0u;
    __syncthreads();
    const double sigma = p.sigma[snr], n0 = p.n0[snr];
    const long s0 = (long)blockIdx.x * POL_SYM_PER_BLOCK;
    for (long s = s0 + t; s < p.num_sym && s < s0 + POL_SYM_PER_BLOCK; s += T) {
        const uint64_t trial = p.trial0 + (uint64_t)s;
        // the Monte-Carlo construction's run `trial` at N = nb (polar_construct.hip): message bits, encode, map, noise
        uint32_t r[4];
        polar_synth_mc_info_word(p.seed, trial, 0u, r);
        int u[4], x[4];
        for (int j = 0; j < nb; ++j) u[j] = (int)((r[0] >> j) & 1u);
        if (nb == 1) { x[0] = u[0]; }
        else if (nb == 2) { x[0] = u[0] ^ u[1]; x[1] = u[1]; }
        else { x[0] = u[0] ^ u[1] ^ u[2] ^ u[3]; x[1] = u[2] ^ u[3]; x[2] = u[1] ^ u[3]; x[3] = u[3]; }   // PolarCode.m:855-867
        int sym = 0;
        for (int j = 0; j < nb; ++j) sym += x[j] << j;                                   // Constellation.m:84-93
        const double y = polar_const_point(p.constellation, sym) / p.cnorm + sigma * polar_synth_symbol_noise(p.seed, trial, 0u);
        double l[4];
        polar_synth_bicm_demap(p.constellation, p.cnorm, y, n0, l);                      // Constellation.m:123-144
        double ul[4];
        if (nb == 1) { ul[0] = l[0]; }
        else if (nb == 2) { genie2(l[0], l[1], u[0], ul); }
        else {
            double a[2];
            genie2(cnop_llr(l[0], l[1]), cnop_llr(l[2], l[3]), u[0], ul);
            const int h0 = u[0] ^ u[1], h1 = u[1];                                          // re-encoded first half
            a[0] = vnop_llr((1 - 2 * h0) * l[0], l[1]);
            a[1] = vnop_llr((1 - 2 * h1) * l[2], l[3]);
            genie2(a[0], a[1], u[2], ul + 2);
        }
        for (int j = 0; j < nb; ++j) {
            double v = ul[j];
            v = (v != v) ? -100.0 : (v < -100.0 ? -100.0 : v);                            // MATLAB max drops NaN
            v = v < 100.0 ? v : 100.0;
            int b = (int)floor((v + 100.0) / 0.25);
            b = b < 0 ? 0 : (b >= POLAR_GA_BINS ? POLAR_GA_BINS - 1 : b);
            atomicAdd(&hist[(j * POLAR_GA_BINS + b) * 2 + u[j]], 1u);
        }
    }
    __syncthreads();
    unsigned long long *out = p.counts + (size_t)snr * nbins;
    for (int i = t; i < nbins; i += T)
        if (hist[i]) atomicAdd(out + i, (unsigned long long)hist[i]);
}

// phi_x_table.m: clamp to [0, 100], index round(x / 0.01) (MATLAB round: half away from zero, C round)
__device__ __forceinline__ double phi_tab(const double *fwd, double x) {
    x = x > 0 ? x : 0;
    x = x < 100 ? x : 100;
    return fwd[(int)round(x / 0.01)];
}
// phi_x_inv.m: -log(y) clamped to [0, 100], index round(v / 1e-3 - 0.499)
__device__ __forceinline__ double phi_inv(const unsigned long long *inv, double y) {
    double v = -polar_synth_log(y);
    v = v > 0 ? v : 0;
    v = v < 100 ? v : 100;
    return __longlong_as_double((long long)inv[(int)round(v / 1e-3 - 0.499)]);
}

__global__ __launch_bounds__(T) void ga_construct_kernel(PolarGaConsParams p) {
    __shared__ double part[T];
    const int pt = blockIdx.x, t = threadIdx.x;
    const int N = p.N, M = p.M, nb = p.nb;
    double *a = p.scr + (size_t)pt * 2 * N, *b = a + N;
    double *ch = p.channels + (size_t)pt * N;
    // PolarCode.m:229-238: sub-block k starts from mean LLR k
    for (int i = t; i < N; i += T) a[i] = p.mean_llr[(size_t)pt * nb + i / M];
    __syncthreads();
    // calculate_awgn_polarization.m: channels = [phi_inv(1 - (1 - phi(c1)) (1 - phi(c2))), c1 + c2], c1 / c2 = odd / even
    for (int st = 0; st < p.m; ++st) {
        for (int q = t; q < N / 2; q += T) {
            const int k = q / (M / 2), j = q % (M / 2);
            const double c1 = a[k * M + 2 * j], c2 = a[k * M + 2 * j + 1];
            b[k * M + j] = phi_inv(p.inv, 1 - (1 - phi_tab(p.fwd, c1)) * (1 - phi_tab(p.fwd, c2)));
            b[k * M + M / 2 + j] = c1 + c2;
        }
        __syncthreads();
        double *tmp = a; a = b; b = tmp;
    }
    // PolarCode.m:241-246: bit-reversed per sub-block
    for (int i = t; i < N; i += T) {
        const int k = i / M, j = i % M;
        const int r = p.m ? (int)(__brev((unsigned)j) >> (32 - p.m)) : 0;
        ch[i] = a[k * M + r];
    }
    __syncthreads();
    // stable descending sort (:248, MATLAB sort 'descend' keeps ties in index order): rank = #greater + #equal before
    uint16_t *ord = p.order + (size_t)pt * N;
    for (int i = t; i < N; i += T) {
        const double c = ch[i];
        int rank = 0;
        for (int j = 0; j < N; ++j) {
            const double d = ch[j];
            rank += (d > c) || (d == c && j < i);
        }
        ord[rank] = (uint16_t)i;
    }
    __syncthreads();
    // :252 qfunc(sqrt(c) / sqrt(2)) = erfc(sqrt(c) / 2) / 2, prefix sums along the order: contiguous chunks, then a scan
    // of the chunk sums by one lane
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

}  // namespace

hipError_t polar_launch_ga_capacity(const PolarGaCapParams &p, int n_snr, hipStream_t st) {
    hipLaunchKernelGGL(ga_capacity_kernel, dim3(p.kind == 2 ? 1 : p.nb, n_snr), dim3(T), 0, st, p);
    return hipGetLastError();
}
hipError_t polar_launch_ga_phi(double *fwd, unsigned long long *inv, double dx, long nx, hipStream_t st) {
    const long lanes = std::max<long>((nx + PHI_RUN - 1) / PHI_RUN, POLAR_GA_PHI_FWD);
    hipLaunchKernelGGL(ga_phi_kernel, dim3((unsigned)((lanes + T - 1) / T)), dim3(T), 0, st, fwd, inv, dx, nx);
    return hipGetLastError();
}
hipError_t polar_launch_ga_polarized(const PolarGaPolParams &p, int n_snr, hipStream_t st) {
    const long blocks = (p.num_sym + POL_SYM_PER_BLOCK - 1) / POL_SYM_PER_BLOCK;
    hipLaunchKernelGGL(ga_polarized_kernel, dim3((unsigned)blocks, n_snr), dim3(T), 0, st, p);
    return hipGetLastError();
}
hipError_t polar_launch_ga_construct(const PolarGaConsParams &p, int n_points, hipStream_t st) {
    hipLaunchKernelGGL(ga_construct_kernel, dim3(n_points), dim3(T), 0, st, p);
    return hipGetLastError();
}
