// polar_mlc.cpp — host side of the MLC receiver (include/polar_amd.h POLAR_RX_MLC, polar_kernels_mlc.hip): checks, parameter fill, dispatch, entry points
#include "polar_host.h"

int polar_host::mlc_check(const polar_code *h, int constellation, int *cid) {
    const int c = constellation & ~POLAR_RX_MLC;
    const int nb = (c & ~0xFF) ? 0 : polar_const_nbits(c);
    if (nb == 0) return fail(POLAR_E_ARG, "unknown constellation %d", c);
    if (h->crc > 0) return fail(POLAR_E_ARG, "the MLC receiver has no CRC (crc_size = %d; PolarM main_MC_CC_Comparison.m:55-62)", h->crc);
    const int M = h->N / nb;
    if (M * nb != h->N || M < 2 || (M & (M - 1)))
        return fail(POLAR_E_ARG, "MLC: N = %d is not %d component codes of a power-of-two length >= 2", h->N, nb);
    *cid = c;
    return POLAR_OK;
}

void polar_host::fill_mlc(const polar_code *h, int cid, double snr_db, PolarMlcParams &p) {
    memset(&p, 0, sizeof p);
    p.n = h->n; p.N = h->N; p.K = h->K;
    p.nb = polar_const_nbits(cid);
    p.M = h->N / p.nb;
    while ((1 << p.m) < p.M) ++p.m;
    p.constellation = cid;
    p.sigma = sigma_of_snr_db(snr_db);                                  // main_MC_CC_Comparison.m:90
    p.n0 = p.sigma * p.sigma;
    p.cnorm = polar_const_norm(cid);
    p.stride = 1;
    p.info_block_div = 1;                                               // fresh info every run (:50)
    p.frozen = h->d_frozen.p; p.order = h->d_order.p;
}

// Dispatch as decode_sc_p1 (small batches one codeword per wave, state in LDS; larger ones one lane per codeword; same doubles),
// with the crossover at eight codewords per resident wave instead of four: the demapper adds fp64 VALU work to every layer
// (2.2x / 3.8x the VALU instructions of decode_sc_p1's kernel at N = 2048 for 4- / 16-ASK), which a lane-per-codeword launch
// of few waves cannot hide (N = 2048, B = 4096: 12.9 / 15.7 ms one lane per codeword, 8.8 / 7.0 ms one codeword per wave).
int polar_host::mlc_decode_launch(polar_code *h, int cid, const double *d_y, double n0, long B, const unsigned int *n_dev,
                                  double *d_out, uint8_t *d_out_bytes, hipStream_t st) {
    h->last_lat_waves = 0; h->last_lane_waves = 0;
    PolarMlcParams p;
    fill_mlc(h, cid, 0.0, p);
    p.n0 = n0; p.B = B; p.n_dev = n_dev; p.y = const_cast<double *>(d_y); p.out = d_out; p.out_bytes = d_out_bytes;
    const size_t lds = polar_mlc_lat_lds_bytes(h->N, p.nb);
    const long lat_waves = lds <= h->lds_per_block ? (long)h->num_cu * std::max<long>(1, (long)(h->lds_per_block / lds)) : 0;
    const long lat_max = h->knobs.lat_max_b < 0 ? 0 : (h->knobs.lat_max_b ? h->knobs.lat_max_b : lat_waves * 8);
    if (lat_waves > 0 && B <= lat_max) {
        HIP_TRY(polar_launch_mlc_sc_lat(p, lat_grid(h, std::min<long>(B, lat_waves)), st));
    } else {
        const size_t per = polar_mlc_scr_doubles(h->N, p.nb);
        int grid = 1;
        int rc = grid_that_fits(h, lane_grid(h, std::min<long>((B + 63) / 64, (long)h->num_cu * 16)), per * sizeof(double),
                                [&](int g) { return h->d_llr_scr.ensure((size_t)g * per + 64); }, &grid);
        if (rc) return rc;
        p.scr = h->d_llr_scr.p;
        HIP_TRY(polar_launch_mlc_sc(p, grid, st));
        h->last_lane_waves = grid;
    }
    return POLAR_OK;
}

// the argument checks of the MLC entry points (ptrs_set: none of the call's own pointers is null); the caller returns at B == 0
static int mlc_args(const polar_code *h, bool ptrs_set, int constellation, long B, int *cid) {
    return check_args(h && ptrs_set, kNoList, B, [&] { return mlc_check(h, constellation, cid); });
}

extern "C" {

int polar_decode_mlc_dev(polar_code_t *h, int constellation, const double *d_y, double n0, long B, double *d_out, void *stream) {
    int cid, rc;
    if ((rc = mlc_args(h, d_y && d_out, constellation, B, &cid)) || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    return mlc_decode_launch(h, cid, d_y, n0, B, nullptr, d_out, nullptr, (hipStream_t)stream);
}

int polar_decode_mlc(polar_code_t *h, int constellation, const double *y, double n0, long B, double *out) {
    int cid, rc;
    if ((rc = mlc_args(h, y && out, constellation, B, &cid)) || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    const size_t M = (size_t)(h->N / polar_const_nbits(cid));
    if ((rc = h->d_in.ensure((size_t)B * M + (size_t)B * h->K))) return rc;
    double *d_out = h->d_in.p + (size_t)B * M;
    HIP_TRY(hipMemcpy(h->d_in.p, y, (size_t)B * M * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = mlc_decode_launch(h, cid, h->d_in.p, n0, B, nullptr, d_out, nullptr, nullptr))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_out, (size_t)B * h->K * sizeof(double), hipMemcpyDeviceToHost));
    return POLAR_OK;
}

int polar_encode_mlc(polar_code_t *h, int constellation, const uint8_t *info, long B, uint8_t *coded) {
    int cid, rc;
    if ((rc = mlc_args(h, info && coded, constellation, B, &cid)) || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    if ((rc = h->d_bytes_a.ensure((size_t)B * h->K))) return rc;
    if ((rc = h->d_bytes_b.ensure((size_t)B * h->N))) return rc;
    HIP_TRY(hipMemcpy(h->d_bytes_a.p, info, (size_t)B * h->K, hipMemcpyHostToDevice));
    PolarMlcParams p;
    fill_mlc(h, cid, 0.0, p);
    p.B = B; p.info = h->d_bytes_a.p; p.coded = h->d_bytes_b.p;
    HIP_TRY(polar_launch_mlc_front(p, 0, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(coded, h->d_bytes_b.p, (size_t)B * h->N, hipMemcpyDeviceToHost));
    return POLAR_OK;
}

int polar_synth_mlc_dev(polar_code_t *h, int constellation, uint64_t seed, uint64_t trial0, long B, double snr_db,
                        double *d_y, uint8_t *d_info, void *stream) {
    int cid, rc;
    if ((rc = mlc_args(h, d_y, constellation, B, &cid)) || B == 0) return rc;
    DevGuard dg_;
    if ((rc = ensure_device(h, dg_))) return rc;
    PolarMlcParams p;
    fill_mlc(h, cid, snr_db, p);
    p.B = B; p.seed = seed; p.trial0 = trial0; p.y = d_y; p.info_out = d_info;
    HIP_TRY(polar_launch_mlc_front(p, 0, (hipStream_t)stream));
    return POLAR_OK;
}

}  // extern "C"
