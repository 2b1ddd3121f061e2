// polar_rm.h — launch interface of the rate-matching kernels (polar_kernels_rm.hip; include/polar_amd.h polar_set_rate_match ...,
// DESIGN.md §8k), in a header of its own: polar_kernels.h, which every kernel translation unit is fingerprinted on, stays as it is.
//
// The pattern on the device is its INVERSE: per coded position p a descriptor of two words, desc[2 p] = the number of transmit
// positions e with sel[e] = p, bit 31 set for a known position; desc[2 p + 1] = that e itself where there is one, else the offset of
// the position's sources in `src` (ascending e).
#pragma once
#include "polar_kernels.h"

constexpr uint32_t kRmKnown = 0x80000000u;

struct PolarRmParams {
    int N, E;
    long B;
    const uint32_t *desc;        // [N][2] device
    const uint32_t *src;         // [E] device: the sources of every position, position by position, ascending e
    int max_src;                 // the largest source count of a position
    double short_llr;
};
// tx[b][e] = coded[b][sel[e]]
hipError_t polar_launch_rm_select(const uint8_t *coded, const uint16_t *sel, long B, int N, int E, uint8_t *tx, hipStream_t st);
// llr[b][p] = short_llr at a known position, else +0.0 + widen(rx[b][e0]) + widen(rx[b][e1]) + ... over the sources of p
hipError_t polar_launch_rm_recover(const PolarRmParams &p, const void *rx, int fmt, double *llr, hipStream_t st);
// the channel of the workload over GIVEN transmit bits: rx[b][e] = polar_synth_llr(s, tx[b][e], z), z = element e & 1 of
// polar_synth_noise_pair(seed, trial0 + b * stride, e >> 1)
hipError_t polar_launch_rm_channel(const uint8_t *tx, long B, int E, uint64_t seed, uint64_t trial0, long stride, double s, double *rx,
                                   hipStream_t st);
// the counters of the sweep (include/polar_amd.h POLAR_RM_*): decoded / sent info [B][K]; ctr[0 .. POLAR_RM_N) are ADDED to
hipError_t polar_launch_rm_classify(const uint8_t *dec, const uint8_t *sent, long B, int K, unsigned long long *ctr, hipStream_t st);
// ga_construct_kernel (polar_kernels_ga.hip) with one block of N started from init [n_points][N] in coded order; the leaves with
// forced[leaf] != 0 (device uint8 [N] or nullptr) go to the end of the order in ascending index
struct PolarRmGaParams {
    int n, N;
    const double *init;          // [n_points][N]
    const uint8_t *forced;       // [N] or nullptr
    const double *fwd;           // phi tables (polar_launch_ga_phi)
    const unsigned long long *inv;
    double *scr;                 // [n_points][2][N]
    double *channels;            // [n_points][N]
    uint16_t *order;             // [n_points][N]
    double *prefix;              // [n_points][N]
};
hipError_t polar_launch_rm_ga_construct(const PolarRmGaParams &p, int n_points, hipStream_t st);
