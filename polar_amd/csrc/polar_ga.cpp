// polar_ga.cpp — Gaussian-approximation code construction (PolarM/PolarCode.m:198-255) and the capacity helpers it rests
// on (Constellation.m:190-370, CapacityHelper/, GaussianApproximation/): host side of polar_kernels_ga.hip. No handle.
// DESIGN.md §8b.
#include "polar_host.h"

using namespace polar_host;

namespace {

constexpr int kBpskTab = 4001;              // bpsk_cap.mat: snr_vec_db = -20 : 0.01 : 20 as s_k = -20 + k * 0.01
constexpr long kPolarizedSym = 250000;      // Constellation.m:300
constexpr int kMaxSnrPerLaunch = 65535;     // grid.y

bool ga_constellation_ok(int c) {
    return c == POLAR_CONST_BPSK || c == POLAR_CONST_ASK4_GRAY || c == POLAR_CONST_ASK4_SP || c == POLAR_CONST_ASK16_GRAY ||
           c == POLAR_CONST_ASK16_SP;
}

int check_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(POLAR_E_DEVICE, "no HIP device: the GA construction has no CPU path");
    return POLAR_OK;
}

// y grid of the integrals: y_k = -ymax + k * dy, k = 0 .. P-1, P = floor(2 ymax / dy + 1e-9) + 1
PolarGaGrid make_grid(double n0, double ymax, double dy) {
    PolarGaGrid g;
    g.n0 = n0; g.ymax = ymax; g.dy = dy;
    g.P = (long)std::floor(2 * ymax / dy + 1e-9) + 1;
    return g;
}

// kind 0 / 1: get_bicm_capacity (dy = 0.1 sigma) / get_mlc_capacity (dy = 0.01 sigma), ymax = max(points) + 6 sigma + 1;
// kind 2: get_bpsk_cap (n0 = 10^(-snr/10) / 2, dy = 0.001 sqrt(n0), ymax = min(10000, 1 + 3 + 3 sqrt(n0)))
int capacity(int kind, int c, const double *snr_db, int n, double *out) {
    if (!snr_db || !out || n < 0) return fail(POLAR_E_ARG, "NULL argument or negative count");
    if (kind != 2 && !ga_constellation_ok(c))
        return fail(POLAR_E_ARG, "constellation %d not supported by the GA construction (BPSK, 4-ASK, 16-ASK)", c);
    if (n == 0) return POLAR_OK;
    int rc;
    if ((rc = check_device())) return rc;
    PolarGaCapParams p;
    std::memset(&p, 0, sizeof p);
    p.kind = kind;
    p.nb = kind == 2 ? 1 : polar_const_nbits(c);
    p.ns = 1 << p.nb;
    double pmax = -1e300;
    if (kind != 2) {
        const double norm = polar_const_norm(c);
        for (int s = 0; s < p.ns; ++s) { p.pt[s] = polar_const_point(c, s) / norm; pmax = std::max(pmax, p.pt[s]); }
    }
    std::vector<PolarGaGrid> g(n);
    for (int i = 0; i < n; ++i) {
        if (kind == 2) {
            const double n0 = 1.0 / 2 * std::pow(10.0, -snr_db[i] / 10);
            g[i] = make_grid(n0, std::min(10000.0, 1.0 + 3 + 3 * std::sqrt(n0)), std::sqrt(n0) * 0.001);
        } else {
            const double s = sigma_of_snr_db(snr_db[i]);
            g[i] = make_grid(s * s, pmax + 6 * s + 1, s * (kind == 0 ? 0.1 : 0.01));
        }
        if (!(g[i].P > 0 && g[i].P < (1L << 40))) return fail(POLAR_E_ARG, "SNR %g dB gives an unusable grid", snr_db[i]);
    }
    DevBuf<PolarGaGrid> d_g;
    DevBuf<double> d_out;
    struct Guard { DevBuf<PolarGaGrid> &a; DevBuf<double> &b; ~Guard() { a.release(); b.release(); } } guard{d_g, d_out};
    if ((rc = d_g.ensure(n))) return rc;
    if ((rc = d_out.ensure((size_t)n * p.nb))) return rc;
    HIP_TRY(hipMemcpy(d_g.p, g.data(), (size_t)n * sizeof(PolarGaGrid), hipMemcpyHostToDevice));
    for (int i0 = 0; i0 < n; i0 += kMaxSnrPerLaunch) {
        p.grid = d_g.p + i0;
        p.out = d_out.p + (size_t)i0 * p.nb;
        HIP_TRY(polar_launch_ga_capacity(p, std::min(kMaxSnrPerLaunch, n - i0), nullptr));
    }
    HIP_TRY(hipMemcpy(out, d_out.p, (size_t)n * p.nb * sizeof(double), hipMemcpyDeviceToHost));
    return POLAR_OK;
}

// the BPSK capacity table of get_bpsk_llr_for_capacity.m, computed once per process
std::mutex g_tab_mu;
std::vector<double> g_bpsk_tab;

int bpsk_table(std::vector<double> &tab) {
    std::lock_guard<std::mutex> lk(g_tab_mu);
    if (g_bpsk_tab.empty()) {
        std::vector<double> snr(kBpskTab), cap(kBpskTab);
        for (int k = 0; k < kBpskTab; ++k) snr[k] = -20.0 + k * 0.01;
        int rc = capacity(2, 0, snr.data(), kBpskTab, cap.data());
        if (rc) return rc;
        g_bpsk_tab = cap;
    }
    tab = g_bpsk_tab;
    return POLAR_OK;
}

int polarized_counts(int c, const double *snr_db, int n, long num_sym, uint64_t seed, uint64_t trial0, uint64_t *counts) {
    if (!snr_db || !counts || n < 0 || num_sym < 0) return fail(POLAR_E_ARG, "NULL argument or negative count");
    if (!ga_constellation_ok(c))
        return fail(POLAR_E_ARG, "constellation %d not supported by the polarized capacity (BPSK, 4-ASK, 16-ASK)", c);
    if (n == 0 || num_sym == 0) return POLAR_OK;
    int rc;
    if ((rc = check_device())) return rc;
    const int nb = polar_const_nbits(c);
    const size_t per = (size_t)nb * POLAR_GA_BINS * 2;
    std::vector<double> sg(n), n0(n);
    for (int i = 0; i < n; ++i) { sg[i] = sigma_of_snr_db(snr_db[i]); n0[i] = sg[i] * sg[i]; }
    DevBuf<double> d_s;
    DevBuf<unsigned long long> d_c;
    struct Guard { DevBuf<double> &a; DevBuf<unsigned long long> &b; ~Guard() { a.release(); b.release(); } } guard{d_s, d_c};
    if ((rc = d_s.ensure((size_t)2 * n))) return rc;
    if ((rc = d_c.ensure((size_t)n * per))) return rc;
    HIP_TRY(hipMemcpy(d_s.p, sg.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_s.p + n, n0.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_c.p, 0, (size_t)n * per * sizeof(unsigned long long)));
    PolarGaPolParams p;
    p.constellation = c; p.nb = nb; p.cnorm = polar_const_norm(c);
    p.seed = seed; p.trial0 = trial0; p.num_sym = num_sym;
    for (int i0 = 0; i0 < n; i0 += kMaxSnrPerLaunch) {
        p.sigma = d_s.p + i0; p.n0 = d_s.p + n + i0;
        p.counts = d_c.p + (size_t)i0 * per;
        HIP_TRY(polar_launch_ga_polarized(p, std::min(kMaxSnrPerLaunch, n - i0), nullptr));
    }
    std::vector<unsigned long long> h((size_t)n * per);
    HIP_TRY(hipMemcpy(h.data(), d_c.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < h.size(); ++i) counts[i] += (uint64_t)h[i];
    return POLAR_OK;
}

}  // namespace

extern "C" {

int polar_bicm_capacity(int constellation, const double *snr_db, int n, double *out) {
    return capacity(0, constellation, snr_db, n, out);
}
int polar_mlc_capacity(int constellation, const double *snr_db, int n, double *out) {
    return capacity(1, constellation & ~POLAR_RX_MLC, snr_db, n, out);
}
int polar_bpsk_capacity(const double *snr_db, int n, double *out) { return capacity(2, 0, snr_db, n, out); }

int polar_ga_phi_tables(double phi_dx, double *fwd, double *inv) {
    if (!fwd || !inv) return fail(POLAR_E_ARG, "NULL argument");
    if (!(phi_dx >= 1e-7 && phi_dx <= 1.0)) return fail(POLAR_E_ARG, "phi_dx = %g out of range [1e-7, 1]", phi_dx);
    int rc;
    if ((rc = check_device())) return rc;
    DevBuf<double> d_f;
    DevBuf<unsigned long long> d_i;
    struct Guard { DevBuf<double> &a; DevBuf<unsigned long long> &b; ~Guard() { a.release(); b.release(); } } guard{d_f, d_i};
    if ((rc = d_f.ensure(POLAR_GA_PHI_FWD))) return rc;
    if ((rc = d_i.ensure(POLAR_GA_PHI_INV))) return rc;
    HIP_TRY(hipMemset(d_i.p, 0, POLAR_GA_PHI_INV * sizeof(unsigned long long)));
    HIP_TRY(polar_launch_ga_phi(d_f.p, d_i.p, phi_dx, (long)std::floor(400 / phi_dx + 1e-6) + 1, nullptr));
    HIP_TRY(hipMemcpy(fwd, d_f.p, POLAR_GA_PHI_FWD * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(inv, d_i.p, POLAR_GA_PHI_INV * sizeof(double), hipMemcpyDeviceToHost));
    return POLAR_OK;
}

int polar_polarized_counts(int constellation, const double *snr_db, int n, long num_sym, uint64_t seed, uint64_t trial0,
                           uint64_t *counts) {
    return polarized_counts(constellation, snr_db, n, num_sym, seed, trial0, counts);
}

int polar_polarized_capacity_from_counts(int constellation, int n, const uint64_t *counts, double *out) {
    if (!counts || !out || n < 0) return fail(POLAR_E_ARG, "NULL argument or negative count");
    if (!ga_constellation_ok(constellation)) return fail(POLAR_E_ARG, "unknown constellation %d", constellation);
    const int nb = polar_const_nbits(constellation);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < nb; ++j) {
            // Constellation.m:336-365: histogram entropies, cap = h_y - h_y_u, min(cap, 1)
            const uint64_t *c = counts + ((size_t)i * nb + j) * POLAR_GA_BINS * 2;
            double tot = 0, n0 = 0, n1 = 0;
            for (int b = 0; b < POLAR_GA_BINS; ++b) { n0 += (double)c[2 * b]; n1 += (double)c[2 * b + 1]; }
            tot = n0 + n1;
            double hy = 0, hu = 0;
            for (int b = 0; b < POLAR_GA_BINS; ++b) {
                const double py = (double)(c[2 * b] + c[2 * b + 1]) / tot, p0 = (double)c[2 * b] / n0, p1 = (double)c[2 * b + 1] / n1;
                if (py > 0) hy = hy + std::log2(py) * py * (-1);
                if (p0 > 0) hu = hu + 0.5 * std::log2(p0) * p0 * (-1);
                if (p1 > 0) hu = hu + 0.5 * std::log2(p1) * p1 * (-1);
            }
            const double cap = hy - hu;
            out[(size_t)i * nb + j] = std::isnan(cap) ? 1.0 : std::min(cap, 1.0);
        }
    return POLAR_OK;
}

int polar_polarized_capacity(int constellation, const double *snr_db, int n, long num_sym, uint64_t seed, double *out) {
    if (!out) return fail(POLAR_E_ARG, "NULL argument");
    if (!ga_constellation_ok(constellation)) return fail(POLAR_E_ARG, "unknown constellation %d", constellation);
    if (n <= 0) return n < 0 ? fail(POLAR_E_ARG, "negative count") : POLAR_OK;
    const int nb = polar_const_nbits(constellation);
    std::vector<uint64_t> cnt((size_t)n * nb * POLAR_GA_BINS * 2, 0);
    int rc = polarized_counts(constellation, snr_db, n, num_sym, seed, 0, cnt.data());
    if (rc) return rc;
    return polar_polarized_capacity_from_counts(constellation, n, cnt.data(), out);
}

int polar_ga_mean_llr(const double *capacity, int n, double *mean_llr) {
    if (!capacity || !mean_llr || n < 0) return fail(POLAR_E_ARG, "NULL argument or negative count");
    std::vector<double> tab;
    int rc = bpsk_table(tab);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        // get_bpsk_llr_for_capacity.m: the first entry reaching the capacity, else (no break) the last one
        int k = 0;
        for (; k < kBpskTab - 1; ++k)
            if (tab[k] >= capacity[i]) break;
        mean_llr[i] = 4 * std::pow(10.0, (-20.0 + k * 0.01) / 10);
    }
    return POLAR_OK;
}

int polar_ga_construction(int n, int constellation, const double *snr_db, int n_points, double phi_dx, uint64_t seed,
                          const double *capacity_in, double *channels, uint16_t *order, double *bler_prefix) {
    const bool mlc = constellation & POLAR_RX_MLC;
    const int c = constellation & ~POLAR_RX_MLC;
    if (n < 1 || n > POLAR_MAX_N_LOG2) return fail(POLAR_E_ARG, "n = %d out of range [1, %d]", n, POLAR_MAX_N_LOG2);
    if (!ga_constellation_ok(c))
        return fail(POLAR_E_ARG, "constellation %d not supported by the GA construction (BPSK, 4-ASK, 16-ASK)", c);
    if (n_points < 0 || (n_points && !snr_db && !capacity_in)) return fail(POLAR_E_ARG, "NULL argument or negative count");
    if (!(phi_dx >= 1e-7 && phi_dx <= 1.0)) return fail(POLAR_E_ARG, "phi_dx = %g out of range [1e-7, 1]", phi_dx);
    const int N = 1 << n, nb = polar_const_nbits(c);
    if (N / nb < 2) return fail(POLAR_E_ARG, "N / n_bits = %d / %d is below 2", N, nb);
    if (n_points == 0) return POLAR_OK;
    if (!capacity_in && !snr_db) return fail(POLAR_E_ARG, "NULL snr_db");
    int rc;
    if ((rc = check_device())) return rc;
    // PolarCode.m:202-214: capacity per bit-channel
    std::vector<double> cap((size_t)n_points * nb);
    if (capacity_in) std::memcpy(cap.data(), capacity_in, cap.size() * sizeof(double));
    else if (mlc) rc = capacity(1, c, snr_db, n_points, cap.data());
    else if (nb == 1) rc = capacity(0, c, snr_db, n_points, cap.data());
    else rc = polar_polarized_capacity(c, snr_db, n_points, kPolarizedSym, seed, cap.data());
    if (rc) return rc;
    std::vector<double> llr(cap.size());
    if ((rc = polar_ga_mean_llr(cap.data(), (int)cap.size(), llr.data()))) return rc;
    const int M = N / nb, m = n - (nb == 1 ? 0 : (nb == 2 ? 1 : 2));
    DevBuf<double> d_f, d_llr, d_scr, d_ch, d_pre;
    DevBuf<unsigned long long> d_i;
    DevBuf<uint16_t> d_ord;
    struct Guard {
        DevBuf<double> &a, &b, &c, &d, &e; DevBuf<unsigned long long> &f; DevBuf<uint16_t> &g;
        ~Guard() { a.release(); b.release(); c.release(); d.release(); e.release(); f.release(); g.release(); }
    } guard{d_f, d_llr, d_scr, d_ch, d_pre, d_i, d_ord};
    if ((rc = d_f.ensure(POLAR_GA_PHI_FWD))) return rc;
    if ((rc = d_i.ensure(POLAR_GA_PHI_INV))) return rc;
    if ((rc = d_llr.ensure(llr.size()))) return rc;
    if ((rc = d_scr.ensure((size_t)n_points * 2 * N))) return rc;
    if ((rc = d_ch.ensure((size_t)n_points * N))) return rc;
    if ((rc = d_pre.ensure((size_t)n_points * N))) return rc;
    if ((rc = d_ord.ensure((size_t)n_points * N))) return rc;
    // initialize_phi(phi_dx)
    HIP_TRY(hipMemset(d_i.p, 0, POLAR_GA_PHI_INV * sizeof(unsigned long long)));
    HIP_TRY(polar_launch_ga_phi(d_f.p, d_i.p, phi_dx, (long)std::floor(400 / phi_dx + 1e-6) + 1, nullptr));
    HIP_TRY(hipMemcpy(d_llr.p, llr.data(), llr.size() * sizeof(double), hipMemcpyHostToDevice));
    PolarGaConsParams p;
    p.m = m; p.M = M; p.nb = nb; p.N = N;
    p.mean_llr = d_llr.p; p.fwd = d_f.p; p.inv = d_i.p; p.scr = d_scr.p;
    p.channels = d_ch.p; p.order = d_ord.p; p.prefix = d_pre.p;
    HIP_TRY(polar_launch_ga_construct(p, n_points, nullptr));
    const size_t tot = (size_t)n_points * N;
    if (channels) HIP_TRY(hipMemcpy(channels, d_ch.p, tot * sizeof(double), hipMemcpyDeviceToHost));
    if (order) HIP_TRY(hipMemcpy(order, d_ord.p, tot * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (bler_prefix) HIP_TRY(hipMemcpy(bler_prefix, d_pre.p, tot * sizeof(double), hipMemcpyDeviceToHost));
    if (!channels && !order && !bler_prefix) HIP_TRY(hipDeviceSynchronize());
    return POLAR_OK;
}

}  // extern "C"
