// polar_bicm.cpp — the reference's Constellation class beside PolarCode (PolarM/Constellation.m): modulate (:84-93) on the host,
// compute_llr_bicm (:123-144) on the device (bicm_demap_kernel, polar_channel.hip), and the symbol-domain BICM receiver —
// decode_scl_llr from received symbols: the LLR rows are materialised in a buffer the handle owns and decode_impl runs
// unchanged (its fallback passes, the folded list-size-1 visits and the latency kernels re-read the raw rows). DESIGN.md §8c.
#include "polar_host.h"

using namespace polar_host;

namespace {

int known_constellation(int c) { return (c & ~0xFF) ? 0 : polar_const_nbits(c); }

int check_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(POLAR_E_DEVICE, "no HIP device: the BICM demapper has no CPU path");
    return POLAR_OK;
}

int demap_args(int constellation, const void *y, int N, long B, double n0, const double *llr, const double *p1) {
    if (!y || (!llr && !p1)) return fail(POLAR_E_ARG, "NULL argument (y, or both of llr and p1)");
    int rc;
    if ((rc = bicm_check(constellation, n0))) return rc;
    if (N < 1 || N > (1 << POLAR_MAX_N_LOG2)) return fail(POLAR_E_ARG, "row length %d out of range [1, %d]", N, 1 << POLAR_MAX_N_LOG2);
    if (B < 0) return fail(POLAR_E_ARG, "negative batch");
    return POLAR_OK;
}

int demap_dev(int constellation, const void *d_y, int y_f32, int N, long B, double n0, double *d_llr, double *d_p1, void *stream) {
    int rc;
    if ((rc = demap_args(constellation, d_y, N, B, n0, d_llr, d_p1))) return rc;
    if (B == 0) return POLAR_OK;
    if ((rc = check_device())) return rc;
    PolarDemapParams p;
    fill_demap(constellation, N, n0, p);
    p.B = B; p.y = d_y; p.y_f32 = y_f32; p.llr = d_llr; p.p1 = d_p1;
    HIP_TRY(polar_launch_bicm_demap(p, (hipStream_t)stream));
    return POLAR_OK;
}

// host pointers: rows in pieces of at most 64 MiB of output each, so that device memory use does not grow with B
int demap_host(int constellation, const void *y, int y_f32, int N, long B, double n0, double *llr, double *p1) {
    int rc;
    if ((rc = demap_args(constellation, y, N, B, n0, llr, p1))) return rc;
    if (B == 0) return POLAR_OK;
    if ((rc = check_device())) return rc;
    const size_t esz = y_f32 ? sizeof(float) : sizeof(double);
    const int M = N / polar_const_nbits(constellation);
    const long step = std::max<long>(1, std::min<long>(B, ((long)64 << 20) / ((long)N * 8)));
    DevBuf<double> d_y, d_llr, d_p1;          // (d_y holds floats or doubles)
    struct Guard { DevBuf<double> &a, &b, &c; ~Guard() { a.release(); b.release(); c.release(); } } guard{d_y, d_llr, d_p1};
    if ((rc = d_y.ensure((size_t)step * std::max(M, 1)))) return rc;
    if (llr && (rc = d_llr.ensure((size_t)step * N))) return rc;
    if (p1 && (rc = d_p1.ensure((size_t)step * N))) return rc;
    PolarDemapParams p;
    fill_demap(constellation, N, n0, p);
    p.y = d_y.p; p.y_f32 = y_f32; p.llr = llr ? d_llr.p : nullptr; p.p1 = p1 ? d_p1.p : nullptr;
    for (long b0 = 0; b0 < B; b0 += step) {
        const long nb = std::min(step, B - b0);
        if (M > 0) HIP_TRY(hipMemcpy(d_y.p, (const char *)y + (size_t)b0 * M * esz, (size_t)nb * M * esz, hipMemcpyHostToDevice));
        p.B = nb;
        HIP_TRY(polar_launch_bicm_demap(p, nullptr));
        if (llr) HIP_TRY(hipMemcpy(llr + (size_t)b0 * N, d_llr.p, (size_t)nb * N * sizeof(double), hipMemcpyDeviceToHost));
        if (p1) HIP_TRY(hipMemcpy(p1 + (size_t)b0 * N, d_p1.p, (size_t)nb * N * sizeof(double), hipMemcpyDeviceToHost));
    }
    return POLAR_OK;
}

int decode_args(const polar_code *h, int constellation, const void *y, double n0, long B, int L, const uint8_t *out) {
    return check_args(h && y && out, L, B, [&] { return bicm_check(constellation, n0); });
}

int decode_dev(polar_code_t *h, int constellation, const void *d_y, int y_f32, double n0, long B, int L, uint8_t *d_out,
               double *d_pm, void *stream) {
    int rc;
    if ((rc = decode_args(h, constellation, d_y, n0, B, L, d_out))) return rc;
    if (B == 0) return POLAR_OK;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    const double *d_llr = nullptr;
    if ((rc = bicm_front(h, constellation, n0, d_y, y_f32, B, (hipStream_t)stream, &d_llr))) return rc;
    return decode_impl(h, d_llr, 0, B, nullptr, L, d_out, d_pm, stream, nullptr, nullptr);
}

int decode_host(polar_code_t *h, int constellation, const void *y, int y_f32, double n0, long B, int L, uint8_t *out) {
    int rc;
    if ((rc = decode_args(h, constellation, y, n0, B, L, out))) return rc;
    const SymRows sym{constellation, h->N / polar_const_nbits(constellation), n0};
    return host_decode(h, y, y_f32, &sym, B, L, out);
}

}  // namespace

int polar_host::bicm_check(int constellation, double n0) {
    if (!known_constellation(constellation)) return fail(POLAR_E_ARG, "unknown constellation %d", constellation);
    if (!(std::isfinite(n0) && n0 > 0)) return fail(POLAR_E_ARG, "noise variance n0 = %g must be finite and > 0", n0);
    return POLAR_OK;
}

void polar_host::fill_demap(int cid, int N, double n0, PolarDemapParams &p) {
    memset(&p, 0, sizeof p);
    p.nb = polar_const_nbits(cid);
    p.N = N; p.M = N / p.nb; p.n0 = n0;
    const double norm = polar_const_norm(cid);
    for (int s = 0; s < (1 << p.nb); ++s) p.pt[s] = polar_const_point(cid, s) / norm;
}

int polar_host::bicm_front(polar_code *c, int cid, double n0, const void *d_y, int y_f32, long B, hipStream_t st, const double **d_llr) {
    int rc;
    if ((rc = c->d_bicm_llr.ensure((size_t)B * c->N))) return rc;
    PolarDemapParams p;
    fill_demap(cid, c->N, n0, p);
    p.B = B; p.y = d_y; p.y_f32 = y_f32; p.llr = c->d_bicm_llr.p;
    HIP_TRY(polar_launch_bicm_demap(p, st));
    *d_llr = c->d_bicm_llr.p;
    return POLAR_OK;
}

extern "C" {

// Constellation.modulate (Constellation.m:84-93): symbol index = sum 2^j * bit j (LSB first), on the host
int polar_modulate(int constellation, const uint8_t *coded, int N, long B, double *sym) {
    if (!coded || !sym) return fail(POLAR_E_ARG, "NULL argument");
    const int nb = known_constellation(constellation);
    if (!nb) return fail(POLAR_E_ARG, "unknown constellation %d", constellation);
    if (N < 1 || N > (1 << POLAR_MAX_N_LOG2)) return fail(POLAR_E_ARG, "row length %d out of range [1, %d]", N, 1 << POLAR_MAX_N_LOG2);
    if (B < 0) return fail(POLAR_E_ARG, "negative batch");
    const int M = N / nb;
    double pt[16];
    const double norm = polar_const_norm(constellation);
    for (int s = 0; s < (1 << nb); ++s) pt[s] = polar_const_point(constellation, s) / norm;
    for (long b = 0; b < B; ++b)
        for (int i = 0; i < M; ++i) {
            int s = 0;
            for (int j = 0; j < nb; ++j) s += (1 << j) * (coded[(size_t)b * N + (size_t)i * nb + j] & 1);
            sym[(size_t)b * M + i] = pt[s];
        }
    return POLAR_OK;
}

int polar_demap_bicm(int constellation, const double *y, int N, long B, double n0, double *llr, double *p1) {
    return demap_host(constellation, y, 0, N, B, n0, llr, p1);
}
int polar_demap_bicm_f32(int constellation, const float *y, int N, long B, double n0, double *llr, double *p1) {
    return demap_host(constellation, y, 1, N, B, n0, llr, p1);
}
int polar_demap_bicm_dev(int constellation, const double *d_y, int N, long B, double n0, double *d_llr, double *d_p1, void *stream) {
    return demap_dev(constellation, d_y, 0, N, B, n0, d_llr, d_p1, stream);
}
int polar_demap_bicm_dev_f32(int constellation, const float *d_y, int N, long B, double n0, double *d_llr, double *d_p1, void *stream) {
    return demap_dev(constellation, d_y, 1, N, B, n0, d_llr, d_p1, stream);
}

int polar_decode_bicm_batch(polar_code_t *h, int constellation, const double *y, double n0, long B, int L, uint8_t *out) {
    return decode_host(h, constellation, y, 0, n0, B, L, out);
}
int polar_decode_bicm_batch_f32(polar_code_t *h, int constellation, const float *y, double n0, long B, int L, uint8_t *out) {
    return decode_host(h, constellation, y, 1, n0, B, L, out);
}
int polar_decode_bicm_batch_dev(polar_code_t *h, int constellation, const double *d_y, double n0, long B, int L, uint8_t *d_out,
                                double *d_pm, void *stream) {
    return decode_dev(h, constellation, d_y, 0, n0, B, L, d_out, d_pm, stream);
}
int polar_decode_bicm_batch_dev_f32(polar_code_t *h, int constellation, const float *d_y, double n0, long B, int L, uint8_t *d_out,
                                    double *d_pm, void *stream) {
    return decode_dev(h, constellation, d_y, 1, n0, B, L, d_out, d_pm, stream);
}

}  // extern "C"
