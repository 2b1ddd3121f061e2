// polar_sys.h — launch interface of the systematic-coding kernels (polar_kernels_sys.hip; include/polar_amd.h
// polar_encode_sys_batch_dev ...), in a header of its own: polar_kernels.h, which every kernel translation unit is
// fingerprinted on, stays as it is.
//
// A codeword is W = max(1, N / 64) 64-bit words, bit p & 63 of word p >> 6 = position p in natural order; a packed row is W such
// words. Word w of a codeword lives in lane w % 64 (of the codeword's lanes), register w / 64; 64 / W codewords share a wave below
// N = 4096.
#pragma once
#include "polar_kernels.h"

struct PolarSysParams {
    int n, N, K, crc, depth;     // depth: rounds of T^-1 (precode)
    long B;
    const uint64_t *mask;        // [W] packed indicator of the unfrozen set (precode)
    const uint64_t *rows;        // [crc][W] packed: precode — the syndrome rows (H at order[j], and order[K + r]); message — H at order[j] alone
    const uint64_t *dv;          // [crc][W] packed D of the parity positions (precode)
    const uint32_t *qinv;        // [crc] rows of Q^-1 (precode)
    const uint16_t *chk;         // [crc] order[K + r] (message)
    const uint16_t *inv_in;      // [N] position -> index of the input byte that lands there, 0xFFFF: none
    const uint16_t *gather;      // [K] output byte i = bit gather[i] of the word (precode: order, message: msg_u)
    const uint8_t *in;           // [B][K] device
    uint8_t *out;                // [B][K] device or nullptr (precode: u_info)
    uint8_t *coded;              // [B][N] device or nullptr (precode only)
};
hipError_t polar_launch_sys_precode(const PolarSysParams &p, hipStream_t st);
hipError_t polar_launch_sys_message(const PolarSysParams &p, hipStream_t st);
// msg_llr[b][i] = widen(llr[b][pos[i]]) + ext[b][pos[i]]
hipError_t polar_launch_sys_soft(const void *llr, int llr_fmt, const double *ext, const uint16_t *pos, long B, int N, int K,
                                 double *msg_llr, hipStream_t st);
// The systematic workload: the info bits synth_kernel draws for the trials (p.seed, p.trial0, p.stride, p.info_block_div) into
// p.info_out, and the channel of synth_kernel (p.constellation, p.s / p.sigma, p.n0, p.cnorm; the same noise per trial) over GIVEN
// coded bits [B][N] into p.llr
hipError_t polar_launch_sys_draw(const PolarEncodeParams &p, hipStream_t st);
hipError_t polar_launch_sys_channel(const PolarEncodeParams &p, const uint8_t *coded, hipStream_t st);
// The counters of the systematic sweep (include/polar_amd.h POLAR_SY_*): decoded / sent u-domain words and messages [B][K];
// ctr[0 .. POLAR_SY_N) are ADDED to
hipError_t polar_launch_sys_classify(const uint8_t *u_dec, const uint8_t *u_sent, const uint8_t *m_dec, const uint8_t *m_sent, long B,
                                     int K, unsigned long long *ctr, hipStream_t st);
