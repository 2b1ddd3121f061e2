// polar_sys.cpp — systematic polar coding (include/polar_amd.h polar_get_sys_info ... polar_mc_batch_sys): the tables
// (host, bit-packed: T^-1 depth, parity positions, Q^-1, the packed rows of the kernels), built at the first systematic call of a
// handle and dropped by polar_set_crc_matrix; the entry points around polar_kernels_sys.hip; the systematic workload and its sweep.
// No decoder changes: a systematic receiver is any decoder followed by the message kernel.
#include "polar_host.h"
#include "polar_sys.h"

struct SysTables {
    int depth = 0, n_swapped = 0, W = 0;
    std::vector<uint16_t> msg_u, par_u, pos, par;      // [K], [crc], and their coded-row indices
    // what the kernels read
    std::vector<uint64_t> packed;                      // mask [W], syndrome rows [crc][W], CRC rows [crc][W], D [crc][W]
    std::vector<uint32_t> qinv;                        // [crc]
    std::vector<uint16_t> idx;                         // inv_msg [N], inv_info [N], msg_u [K], pos [K], chk [crc]
    DevBuf<uint64_t> d_packed;
    DevBuf<uint32_t> d_qinv;
    DevBuf<uint16_t> d_idx;
    bool uploaded = false;
    // the systematic workload and the host forms: message, precoded word, coded bits, recovered message of a chunk
    DevBuf<uint8_t> d_msg, d_u, d_coded, d_mhat;
    DevBuf<double> d_soft;
};

namespace {

const uint64_t kStage[6] = {0x5555555555555555ull, 0x3333333333333333ull, 0x0F0F0F0F0F0F0F0Full,
                            0x00FF00FF00FF00FFull, 0x0000FFFF0000FFFFull, 0x00000000FFFFFFFFull};

// the encoder's n stages on a packed row
void butterfly(uint64_t *x, int n, int W) {
    for (int it = 0; it < std::min(n, 6); ++it)
        for (int w = 0; w < W; ++w) x[w] ^= (x[w] >> (1 << it)) & kStage[it];
    for (int it = 6; it < n; ++it) {
        const int inc = 1 << (it - 6);
        for (int w = 0; w < W; ++w)
            if (!(w & inc)) x[w] ^= x[w + inc];
    }
}
inline int parity_and(const uint64_t *a, const uint64_t *b, int W) {
    int c = 0;
    for (int w = 0; w < W; ++w) c += __builtin_popcountll(a[w] & b[w]);
    return c & 1;
}
inline void set_bit(uint64_t *x, int p) { x[p >> 6] |= 1ull << (p & 63); }

// depth: the unit vectors of A', 64 at a time as the bits of one word per position (bit-sliced): a round is one butterfly over the
// positions. U_0 = X; U_t = X ^ U_{t-1} ^ T U_{t-1}; the block is solved at the first t >= 1 with T U_t = X
int sys_depth(const polar_code *h) {
    const int N = h->N, n = h->n, Kp = h->K + h->crc;
    std::vector<uint64_t> X(N), U(N), TU(N);
    auto apply_T = [&](const std::vector<uint64_t> &in, std::vector<uint64_t> &out) {
        out = in;
        for (int it = 0; it < n; ++it) {
            const int inc = 1 << it;
            for (int a = 0; a < N; ++a)
                if (!(a & inc)) out[a] ^= out[a + inc];
        }
        for (int a = 0; a < N; ++a)
            if (h->frozen[a]) out[a] = 0;
    };
    int depth = 1;
    for (int c0 = 0; c0 < Kp; c0 += 64) {
        std::fill(X.begin(), X.end(), 0);
        for (int c = c0; c < std::min(Kp, c0 + 64); ++c) X[h->order[c]] |= 1ull << (c - c0);
        U = X;
        apply_T(U, TU);
        int t = 0;
        for (;;) {
            ++t;
            for (int a = 0; a < N; ++a) U[a] = X[a] ^ U[a] ^ TU[a];
            apply_T(U, TU);
            if (TU == X) break;
            if (t > n + 1) return -1;
        }
        depth = std::max(depth, t);
    }
    return depth;
}

int sys_build(polar_code *h) {
    const int N = h->N, n = h->n, K = h->K, crc = h->crc, Kp = K + crc;
    // (the frozen array and `order` of an explicit handle are the caller's: the definitions are on A' = order[0 .. K'))
    for (int i = 0; i < Kp; ++i)
        if (h->order[i] >= N || h->frozen[h->order[i]]) return fail(POLAR_E_ARG, "systematic coding needs order[0 .. K + crc) to be the unfrozen set");
    auto sp = std::make_unique<SysTables>();
    SysTables &t = *sp;
    const int W = t.W = std::max(1, N / 64);
    if ((t.depth = sys_depth(h)) < 0) return fail(POLAR_E_UNSUPPORTED, "T^-1 did not converge");
    t.packed.assign((size_t)W * (1 + 3 * crc), 0);
    uint64_t *mask = t.packed.data(), *sy = mask + W, *hs = sy + (size_t)crc * W, *dv = hs + (size_t)crc * W;
    for (int i = 0; i < Kp; ++i) set_bit(mask, h->order[i]);
    for (int r = 0; r < crc; ++r) {
        for (int j = 0; j < K; ++j)
            if (h->crcm[(size_t)r * K + j] & 1) set_bit(hs + (size_t)r * W, h->order[j]);
        memcpy(sy + (size_t)r * W, hs + (size_t)r * W, (size_t)W * 8);
        set_bit(sy + (size_t)r * W, h->order[K + r]);
    }
    // the parity positions: walk A' from its end
    std::vector<uint64_t> d(W), tu(W), e(W);
    std::vector<uint32_t> cols, basis;
    std::vector<uint8_t> is_par(N, 0);
    for (int i = Kp - 1; i >= 0 && (int)t.par_u.size() < crc; --i) {
        const int p = h->order[i];
        std::fill(e.begin(), e.end(), 0);
        set_bit(e.data(), p);
        d = e;
        for (int k = 0; k < t.depth; ++k) {
            tu = d;
            butterfly(tu.data(), n, W);
            for (int w = 0; w < W; ++w) d[w] = e[w] ^ d[w] ^ (tu[w] & mask[w]);
        }
        uint32_t c = 0;
        for (int r = 0; r < crc; ++r) c |= (uint32_t)parity_and(sy + (size_t)r * W, d.data(), W) << r;
        uint32_t v = c;
        for (uint32_t b : basis) v = std::min(v, v ^ b);
        if (!v) continue;
        basis.push_back(v);
        cols.push_back(c);
        memcpy(dv + t.par_u.size() * (size_t)W, d.data(), (size_t)W * 8);
        t.par_u.push_back((uint16_t)p);
        is_par[p] = 1;
        if (i < K) ++t.n_swapped;
    }
    if ((int)t.par_u.size() != crc) return fail(POLAR_E_UNSUPPORTED, "no %d independent parity positions", crc);
    for (int i = 0; i < Kp; ++i)
        if (!is_par[h->order[i]]) t.msg_u.push_back(h->order[i]);
    // Q^-1 (Gauss-Jordan over GF(2)): row r of Q has bit j = bit r of column j
    std::vector<uint64_t> a(crc);                      // row: Q in the low 32 bits, the identity above
    for (int r = 0; r < crc; ++r) {
        a[r] = 1ull << (32 + r);
        for (int j = 0; j < crc; ++j) a[r] |= (uint64_t)((cols[j] >> r) & 1u) << j;
    }
    for (int col = 0; col < crc; ++col) {
        int piv = col;
        while (piv < crc && !((a[piv] >> col) & 1)) ++piv;
        if (piv == crc) return fail(POLAR_E_UNSUPPORTED, "Q is singular");
        std::swap(a[col], a[piv]);
        for (int r = 0; r < crc; ++r)
            if (r != col && ((a[r] >> col) & 1)) a[r] ^= a[col];
    }
    t.qinv.resize(crc);
    for (int r = 0; r < crc; ++r) t.qinv[r] = (uint32_t)(a[r] >> 32);
    t.pos.resize(K); t.par.resize(crc);
    for (int i = 0; i < K; ++i) t.pos[i] = h->bitrev[t.msg_u[i]];
    for (int r = 0; r < crc; ++r) t.par[r] = h->bitrev[t.par_u[r]];
    t.idx.assign((size_t)2 * N + 2 * K + crc, 0xFFFF);
    for (int i = 0; i < K; ++i) { t.idx[t.msg_u[i]] = (uint16_t)i; t.idx[N + h->order[i]] = (uint16_t)i; }
    for (int i = 0; i < K; ++i) { t.idx[2 * N + i] = t.msg_u[i]; t.idx[2 * N + K + i] = t.pos[i]; }
    for (int r = 0; r < crc; ++r) t.idx[2 * N + 2 * K + r] = h->order[K + r];
    h->sys = sp.release();
    return POLAR_OK;
}

int sys_tables(polar_code *h) { return h->sys ? POLAR_OK : sys_build(h); }

// tables on the device, BEFORE a launch (the handle's device current)
int sys_prepare(polar_code *h) {
    if (int rc = sys_tables(h)) return rc;
    SysTables &t = *h->sys;
    if (t.uploaded) return POLAR_OK;
    int rc;
    if ((rc = upload(t.d_packed, t.packed)) || (rc = upload(t.d_qinv, t.qinv)) || (rc = upload(t.d_idx, t.idx))) return rc;
    t.uploaded = true;
    return POLAR_OK;
}

void sys_params(const polar_code *h, PolarSysParams &p, long B) {
    const SysTables &t = *h->sys;
    memset(&p, 0, sizeof p);
    p.n = h->n; p.N = h->N; p.K = h->K; p.crc = h->crc; p.depth = t.depth; p.B = B;
    p.mask = t.d_packed.p; p.dv = t.d_packed.p + (size_t)t.W * (1 + 2 * h->crc); p.qinv = t.d_qinv.p;
    p.chk = t.d_idx.p + 2 * (size_t)h->N + 2 * (size_t)h->K;
}
int precode_launch(polar_code *h, const uint8_t *d_msg, long B, uint8_t *d_coded, uint8_t *d_u_info, hipStream_t st) {
    PolarSysParams p;
    sys_params(h, p, B);
    p.rows = h->sys->d_packed.p + h->sys->W;
    p.inv_in = h->sys->d_idx.p; p.gather = h->d_order.p;
    p.in = d_msg; p.out = d_u_info; p.coded = d_coded;
    HIP_TRY(polar_launch_sys_precode(p, st));
    return POLAR_OK;
}
int message_launch(polar_code *h, const uint8_t *d_u_info, long R, uint8_t *d_msg, hipStream_t st) {
    PolarSysParams p;
    sys_params(h, p, R);
    p.rows = h->sys->d_packed.p + (size_t)h->sys->W * (1 + h->crc);
    p.inv_in = h->sys->d_idx.p + h->N; p.gather = h->sys->d_idx.p + 2 * (size_t)h->N;
    p.in = d_u_info; p.out = d_msg;
    HIP_TRY(polar_launch_sys_message(p, st));
    return POLAR_OK;
}

int sys_constellation(int constellation, int *cid) {
    if (constellation & POLAR_RX_MLC) return fail(POLAR_E_ARG, "the systematic workload has no MLC receiver");
    if (constellation != 0 && !is_ask_constellation(constellation)) return fail(POLAR_E_ARG, "unknown constellation %d", constellation);
    *cid = constellation == POLAR_CONST_BPSK ? 0 : constellation;
    return POLAR_OK;
}
// the trials' messages into d_msg, their precoded words into d_u, their LLR rows into d_llr (buffers sized by the caller,
// sys_prepare done); `point`: what fill_channel takes — Eb/N0 or SNR in dB —, or with `s_given` (BPSK) the value of p.s itself
int synth_launch(polar_code *h, int cid, uint64_t seed, uint64_t trial0, long stride, long B, double point, bool s_given,
                 double *d_llr, uint8_t *d_msg, uint8_t *d_u, hipStream_t st) {
    SysTables &t = *h->sys;
    PolarEncodeParams p;
    fill_enc(h, p);
    p.B = B; p.seed = seed; p.trial0 = trial0; p.stride = stride;
    fill_channel(h, p, cid, point);
    if (s_given) p.s = point;
    p.llr = d_llr; p.info_out = d_msg;
    HIP_TRY(polar_launch_sys_draw(p, st));
    if (int rc = precode_launch(h, d_msg, B, t.d_coded.p, d_u, st)) return rc;
    HIP_TRY(polar_launch_sys_channel(p, t.d_coded.p, st));
    return POLAR_OK;
}

}  // namespace

void polar_host::sys_release(polar_code *h) {
    if (!h->sys) return;
    SysTables *t = h->sys;
    t->d_packed.release(); t->d_qinv.release(); t->d_idx.release();
    t->d_msg.release(); t->d_u.release(); t->d_coded.release(); t->d_mhat.release(); t->d_soft.release();
    delete t;
    h->sys = nullptr;
}

extern "C" {

int polar_get_sys_info(polar_code_t *h, int *depth, int *n_swapped) {
    if (!h) return fail(POLAR_E_ARG, "NULL handle");
    if (int rc = sys_tables(h)) return rc;
    if (depth) *depth = h->sys->depth;
    if (n_swapped) *n_swapped = h->sys->n_swapped;
    return POLAR_OK;
}
int polar_get_sys_positions(polar_code_t *h, uint16_t *pos, uint16_t *par) {
    if (!h) return fail(POLAR_E_ARG, "NULL handle");
    if (int rc = sys_tables(h)) return rc;
    if (pos) memcpy(pos, h->sys->pos.data(), 2 * (size_t)h->K);
    if (par && h->crc) memcpy(par, h->sys->par.data(), 2 * (size_t)h->crc);
    return POLAR_OK;
}

int polar_encode_sys_batch_dev(polar_code_t *h, const uint8_t *d_msg, long B, uint8_t *d_coded, uint8_t *d_u_info, void *stream) {
    return on_device(h, check_args(h && d_msg && (d_coded || d_u_info), kNoList, B), B, [&]() -> int {
        if (int rc = sys_prepare(h)) return rc;
        return precode_launch(h, d_msg, B, d_coded, d_u_info, (hipStream_t)stream);
    });
}
int polar_encode_sys_batch(polar_code_t *h, const uint8_t *msg, long B, uint8_t *coded, uint8_t *u_info) {
    return on_device(h, check_args(h && msg && (coded || u_info), kNoList, B), B, [&]() -> int {
        int rc;
        if ((rc = sys_prepare(h))) return rc;
        SysTables &t = *h->sys;
        if ((rc = t.d_msg.ensure((size_t)B * h->K)) || (rc = t.d_u.ensure((size_t)B * h->K)) || (rc = t.d_coded.ensure((size_t)B * h->N))) return rc;
        HIP_TRY(hipMemcpy(t.d_msg.p, msg, (size_t)B * h->K, hipMemcpyHostToDevice));
        if ((rc = precode_launch(h, t.d_msg.p, B, coded ? t.d_coded.p : nullptr, u_info ? t.d_u.p : nullptr, nullptr))) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        if ((rc = copy_back(coded, 0, t.d_coded.p, (size_t)B * h->N)) || (rc = copy_back(u_info, 0, t.d_u.p, (size_t)B * h->K))) return rc;
        return POLAR_OK;
    });
}

int polar_sys_message_batch_dev(polar_code_t *h, const uint8_t *d_u_info, long R, uint8_t *d_msg, void *stream) {
    return on_device(h, check_args(h && d_u_info && d_msg, kNoList, R), R, [&]() -> int {
        if (int rc = sys_prepare(h)) return rc;
        return message_launch(h, d_u_info, R, d_msg, (hipStream_t)stream);
    });
}
int polar_sys_message_batch(polar_code_t *h, const uint8_t *u_info, long R, uint8_t *msg) {
    return on_device(h, check_args(h && u_info && msg, kNoList, R), R, [&]() -> int {
        int rc;
        if ((rc = sys_prepare(h))) return rc;
        SysTables &t = *h->sys;
        if ((rc = t.d_u.ensure((size_t)R * h->K))) return rc;
        HIP_TRY(hipMemcpy(t.d_u.p, u_info, (size_t)R * h->K, hipMemcpyHostToDevice));
        if ((rc = message_launch(h, t.d_u.p, R, t.d_u.p, nullptr))) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        return copy_back(msg, 0, t.d_u.p, (size_t)R * h->K);
    });
}

int polar_sys_soft_batch_dev(polar_code_t *h, const void *d_llr, int fmt, const double *d_ext, long B, double *d_msg_llr, void *stream) {
    return on_device(h, check_args(h && d_llr && d_ext && d_msg_llr, kNoList, B, [&] { return llr_fmt_check(fmt, d_llr); }), B, [&]() -> int {
        if (int rc = sys_prepare(h)) return rc;
        HIP_TRY(polar_launch_sys_soft(d_llr, fmt, d_ext, h->sys->d_idx.p + 2 * (size_t)h->N + h->K, B, h->N, h->K, d_msg_llr, (hipStream_t)stream));
        return POLAR_OK;
    });
}
int polar_sys_soft_batch(polar_code_t *h, const void *llr, int fmt, const double *ext, long B, double *msg_llr) {
    return on_device(h, check_args(h && llr && ext && msg_llr, kNoList, B, [&] { return llr_fmt_check(fmt, llr); }), B, [&]() -> int {
        int rc;
        if ((rc = sys_prepare(h))) return rc;
        SysTables &t = *h->sys;
        if ((rc = stage_rows(h, llr, fmt, B))) return rc;
        if ((rc = t.d_soft.ensure((size_t)B * (h->N + h->K)))) return rc;
        HIP_TRY(hipMemcpy(t.d_soft.p, ext, (size_t)B * h->N * sizeof(double), hipMemcpyHostToDevice));
        double *d_out = t.d_soft.p + (size_t)B * h->N;
        HIP_TRY(polar_launch_sys_soft(h->d_in.p, fmt, t.d_soft.p, t.d_idx.p + 2 * (size_t)h->N + h->K, B, h->N, h->K, d_out, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        return copy_back(msg_llr, 0, d_out, (size_t)B * h->K);
    });
}

int polar_synth_sys_llr_dev(polar_code_t *h, int constellation, uint64_t seed, uint64_t trial0, long B, double s_or_snr, double *d_llr,
                            uint8_t *d_msg, uint8_t *d_u_info, void *stream) {
    int cid = 0;
    return on_device(h, check_args(h && d_llr, kNoList, B, [&] { return sys_constellation(constellation, &cid); }), B, [&]() -> int {
        int rc;
        if ((rc = sys_prepare(h))) return rc;
        SysTables &t = *h->sys;
        if ((rc = t.d_coded.ensure((size_t)B * h->N))) return rc;
        if (!d_msg) { if ((rc = t.d_msg.ensure((size_t)B * h->K))) return rc; d_msg = t.d_msg.p; }
        return synth_launch(h, cid, seed, trial0, 1, B, s_or_snr, cid == 0, d_llr, d_msg, d_u_info, (hipStream_t)stream);
    });
}

// Per enabled (list size, point) and per chunk of trials, stream-ordered: the shared walk draws the trials' info bits (they are the
// messages); the precode, the channel over the systematic codeword (the walk's own LLR rows are replaced: same noise), decode_scl_llr,
// the message step, the classification. The counters stay on the device until the end.
int polar_mc_batch_sys(polar_code_t *h, int constellation, uint64_t seed, uint64_t t0, long T, long stride, const double *axis, int n_e,
                       const uint8_t *L, int n_L, const uint8_t *enabled, uint64_t *stats) {
    Sweep sw;
    int rc = sweep_begin(sw, h, axis && L && enabled && stats, "systematic sweep has", constellation, seed, t0, T, stride, axis,
                         n_e > 0 && n_L > 0, stats, [&] { return check_list_sizes(L, n_L); });
    if (rc || T == 0) return rc;
    const int N = h->N, K = h->K;
    const long chunk = sweep_chunk(h, T, (size_t)N * sizeof(double) + (size_t)N + 5 * (size_t)K);
    if ((rc = sys_prepare(h))) return rc;
    SysTables &t = *h->sys;
    if ((rc = sweep_rows(h, chunk)) || (rc = h->d_out.ensure((size_t)chunk * K)) ||
        (rc = t.d_u.ensure((size_t)chunk * K)) || (rc = t.d_coded.ensure((size_t)chunk * N)) || (rc = t.d_mhat.ensure((size_t)chunk * K))) return rc;
    const auto cells = sweep_cells(enabled, n_L, n_e, POLAR_SY_N, std::vector<long>(n_L, chunk));
    return sweep_walk(sw, cells, POLAR_SY_N, n_L, n_e, [&](const SweepCell &cell, long c, const PolarEncodeParams &p) -> int {
        if (int r = precode_launch(h, h->d_bytes_a.p, c, t.d_coded.p, t.d_u.p, nullptr)) return r;
        HIP_TRY(polar_launch_sys_channel(p, t.d_coded.p, nullptr));
        if (int r = decode_impl(h, h->d_in.p, POLAR_LLR_F64, c, nullptr, L[cell.row], h->d_out.p, nullptr, nullptr, nullptr, nullptr)) return r;
        if (int r = message_launch(h, h->d_out.p, c, t.d_mhat.p, nullptr)) return r;
        HIP_TRY(polar_launch_sys_classify(h->d_out.p, t.d_u.p, t.d_mhat.p, h->d_bytes_a.p, c, K, h->d_mc_ctr.p + cell.ctr, nullptr));
        return POLAR_OK;
    });
}

}  // extern "C"
