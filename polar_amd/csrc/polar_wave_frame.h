// polar_wave_frame.h — what the one-codeword-per-wave kernels of the decoder variants share (polar_kernels_flip.hip, _scan.hip,
// _metric.hip) and what the classify kernels of their sweeps share (those three and polar_kernels_adapt.hip): the LDS layout helpers,
// the CRC check on decided bits, the comparison of two words.
//
// A kernel takes a helper from here only where it keeps the machine code it had with the text written out
// (tools/kernel_isa_diff.py against the build before). That holds for straight-line helpers and for a helper that replaces what was
// already a function of the same shape (crc_matches: it reads the parameter struct inside its loops, as the kernels' own functions
// did). A loop that stood in a kernel's body does not survive the move in general — the compiler cleans a kernel up once before it
// inlines, and sees a call there instead of the loop: registers and branch senses come out differently. So the table and row
// loads, the walk over the ops and the counters' epilogue stay written out in every kernel, and the comparison in two of four.
#pragma once
#include "polar_device.h"

namespace {

// 32-bit words of N packed bits
__host__ __device__ inline int packed_words(int N) { return N >= 32 ? N / 32 : 1; }
// first double of layer lam in an array of the layers N, N/2, ..., 1
__device__ __forceinline__ int layer_off(int N, int lam) { return 2 * N - ((2 * N) >> lam); }
__device__ __forceinline__ unsigned get_bit(const uint32_t *w, int i) { return (w[i >> 5] >> (i & 31)) & 1u; }

// do the check bits the CRC matrix gives for the decided info bits equal the decided check bits? p: the kernel's parameters (crc,
// K, crcm, order); bit(pos): the decision at leaf `pos` (wave-uniform result)
template <typename P, typename Bit>
__device__ __forceinline__ bool crc_matches(const P &p, int lane, Bit bit) {
    bool bad = false;
    for (int r = 0; r < p.crc && !bad; ++r) {
        unsigned par = 0;
        for (int j = lane; j < p.K; j += 64) par ^= (unsigned)p.crcm[(size_t)r * p.K + j] & (unsigned)bit(p.order[j]);
        const u64 m = __ballot(par & 1u);
        bad = (unsigned)(__popcll(m) & 1) != (unsigned)bit(p.order[p.K + r]);
    }
    return !bad;
}

// do two words of K bytes differ? (wave-uniform)
__device__ __forceinline__ bool rows_differ(const uint8_t *a, const uint8_t *b, int K, int lane) {
    bool diff = false;
    for (int i = lane; i < K; i += 64) diff |= (a[i] != b[i]);
    return __ballot(diff) != 0;
}

}  // namespace
