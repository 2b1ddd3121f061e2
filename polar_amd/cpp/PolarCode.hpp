// PolarCode.hpp — header-only C++ host mirror of the reference class (PolarC/PolarCode.h:17-36)
// over the C-ABI of include/polar_amd.h. Same constructor and member names, same argument
// meaning; a translation unit written against the reference's PolarCode.h compiles against this
// header unchanged and runs on the MI355X (link with -lpolar_amd). Errors, which the reference
// turns into std::out_of_range / terminate, surface as std::runtime_error carrying
// polar_last_error().
#ifndef POLAR_AMD_POLARCODE_HPP
#define POLAR_AMD_POLARCODE_HPP

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "polar_amd.h"

class PolarCode {
public:
    // PolarCode.h:19-28
    PolarCode(uint8_t num_layers, uint16_t info_length, double epsilon, uint16_t crc_size)
        : _n(num_layers), _info_length(info_length), _crc_size(crc_size) {
        check(polar_create(num_layers, info_length, epsilon, crc_size, &_h));
        _block_length = (uint16_t)(1u << _n);
    }
    // explicit tables (frozen mask, info order, CRC matrix)
    PolarCode(uint8_t num_layers, uint16_t info_length, uint16_t crc_size, const std::vector<uint8_t> &frozen,
              const std::vector<uint16_t> &order, const std::vector<uint8_t> &crc_matrix)
        : _n(num_layers), _info_length(info_length), _crc_size(crc_size) {
        check(polar_create_explicit(num_layers, info_length, crc_size, frozen.data(), order.data(),
                                    crc_size ? crc_matrix.data() : nullptr, &_h));
        _block_length = (uint16_t)(1u << _n);
    }
    ~PolarCode() { polar_destroy(_h); }
    PolarCode(const PolarCode &) = delete;
    PolarCode &operator=(const PolarCode &) = delete;

    // PolarCode.h:30-34
    std::vector<uint8_t> encode(std::vector<uint8_t> info_bits) {
        need(info_bits.size() == _info_length, "encode: info_bits must have info_length entries");
        std::vector<uint8_t> coded(_block_length);
        check(polar_encode(_h, info_bits.data(), coded.data()));
        return coded;
    }
    std::vector<uint8_t> decode_scl_p1(std::vector<double> p1, std::vector<double> p0, uint16_t list_size) {
        need(p1.size() == _block_length && p0.size() == _block_length, "decode_scl_p1: need block_length values");
        std::vector<uint8_t> out(_info_length);
        check(polar_decode_scl_p1(_h, p1.data(), p0.data(), list_size, out.data()));
        return out;
    }
    std::vector<uint8_t> decode_scl_llr(std::vector<double> llr, uint16_t list_size) {
        need(llr.size() == _block_length, "decode_scl_llr: need block_length values");
        std::vector<uint8_t> out(_info_length);
        check(polar_decode_scl_llr(_h, llr.data(), list_size, out.data()));
        return out;
    }
    // PolarM's SC decoder (PolarCode.m:290)
    std::vector<double> decode_sc_p1(std::vector<double> p1) {
        need(p1.size() == _block_length, "decode_sc_p1: need block_length values");
        std::vector<double> out(_info_length);
        check(polar_decode_sc_p1(_h, p1.data(), out.data()));
        return out;
    }
    // batched variant (B codewords, row-major) — the form that fills the GPU
    std::vector<uint8_t> decode_scl_llr_batch(const std::vector<double> &llr, uint16_t list_size) {
        need(llr.size() % _block_length == 0, "decode_scl_llr_batch: size must be a multiple of block_length");
        long B = (long)(llr.size() / _block_length);
        std::vector<uint8_t> out((size_t)B * _info_length);
        check(polar_decode_scl_llr_batch(_h, llr.data(), B, list_size, out.data()));
        return out;
    }
    // single-precision LLRs (B codewords back to back): widened exactly on the device
    std::vector<uint8_t> decode_scl_llr_batch(const std::vector<float> &llr, uint16_t list_size) {
        need(llr.size() % _block_length == 0, "decode_scl_llr_batch: size must be a multiple of block_length");
        const long B = (long)(llr.size() / _block_length);
        std::vector<uint8_t> out((size_t)B * _info_length);
        check(polar_decode_scl_llr_batch_f32(_h, llr.data(), B, list_size, out.data()));
        return out;
    }
    // 16-bit LLRs as raw bit patterns: llr_format = POLAR_LLR_F16 (IEEE binary16) or POLAR_LLR_BF16 (bfloat16), each widened
    // exactly on the device (a quarter of the doubles' bytes on the link)
    std::vector<uint8_t> decode_scl_llr_batch(const std::vector<uint16_t> &llr, int llr_format, uint16_t list_size) {
        need(llr_format == POLAR_LLR_F16 || llr_format == POLAR_LLR_BF16, "decode_scl_llr_batch: 16-bit patterns are POLAR_LLR_F16 or POLAR_LLR_BF16");
        need(llr.size() % _block_length == 0, "decode_scl_llr_batch: size must be a multiple of block_length");
        const long B = (long)(llr.size() / _block_length);
        std::vector<uint8_t> out((size_t)B * _info_length);
        check(polar_decode_scl_llr_batch_fmt(_h, llr.data(), llr_format, B, list_size, out.data()));
        return out;
    }
    // Every path the list decoder holds at the end of each codeword (polar_decode_scl_llr_list_batch; B codewords back to back):
    // rows ordered CRC pass first, then by metric; rows >= n_active are padding; cand row winner[b] is decode_scl_llr's result
    // (winner -1: the all-zero word). Any list size 1 .. POLAR_MAX_LIST.
    struct ListResult {
        long B = 0;
        int L = 0, K = 0;
        std::vector<uint8_t> cand;       // [B][L][K]
        std::vector<double> pm;          // [B][L]
        std::vector<uint8_t> crc_ok;     // [B][L]
        std::vector<int32_t> n_active;   // [B]
        std::vector<int32_t> winner;     // [B]
    };
    ListResult decode_scl_llr_list(const std::vector<double> &llr, uint16_t list_size) {
        need(llr.size() % _block_length == 0, "decode_scl_llr_list: size must be a multiple of block_length");
        need(list_size >= 1 && list_size <= POLAR_MAX_LIST, "decode_scl_llr_list: list size out of range");
        ListResult r;
        r.B = (long)(llr.size() / _block_length); r.L = list_size; r.K = _info_length;
        r.cand.resize((size_t)r.B * r.L * r.K); r.pm.resize((size_t)r.B * r.L); r.crc_ok.resize((size_t)r.B * r.L);
        r.n_active.resize((size_t)r.B); r.winner.resize((size_t)r.B);
        check(polar_decode_scl_llr_list_batch(_h, llr.data(), POLAR_LLR_F64, r.B, r.L, r.cand.data(), r.pm.data(), r.crc_ok.data(),
                                              r.n_active.data(), r.winner.data()));
        return r;
    }
    // The metric the list decoder assigns to given words (polar_path_metric_batch): B codewords back to back, R words of info_length
    // bits per codeword ([B][R][K]; check bits from the CRC matrix) -> [B][R]. Where decode_scl_llr_list holds a word with
    // crc_ok = 1 the value is that row's pm bit for bit.
    std::vector<double> path_metric(const std::vector<double> &llr, const std::vector<uint8_t> &info, int words_per_codeword = 1) {
        need(llr.size() % _block_length == 0, "path_metric: size must be a multiple of block_length");
        const long B = (long)(llr.size() / _block_length);
        need(words_per_codeword >= 1 && words_per_codeword <= POLAR_MAX_LIST, "path_metric: words per codeword out of range");
        need(info.size() == (size_t)B * words_per_codeword * _info_length, "path_metric: info must hold B * R * info_length bits");
        std::vector<double> pm((size_t)B * words_per_codeword);
        check(polar_path_metric_batch(_h, llr.data(), POLAR_LLR_F64, info.data(), B, words_per_codeword, pm.data()));
        return pm;
    }
    // Error analysis of the list decoder over a sweep (polar_mc_batch_list in rounds, as get_bler_quick stops its points: a point
    // leaves once ERR > max_err or RUN >= max_runs). Rounds of `batch` trials; 0: max(256, 2 max_err), then doubling up to 262144.
    // Everything is [list_index * n_points + point_index]; stats additionally * POLAR_LS_N + POLAR_LS_*.
    struct ListStats {
        int n_L = 0, n_points = 0;
        std::vector<uint64_t> stats;
        std::vector<double> bler, miss_rate, undetected_rate, ml_bound;
    };
    ListStats list_stats(const std::vector<double> &axis, const std::vector<uint8_t> &list_size, long max_runs = 1000, long max_err = 100,
                         uint64_t seed = 0, long batch = 0, int constellation = 0) {
        ListStats r;
        r.n_L = (int)list_size.size(); r.n_points = (int)axis.size();
        const size_t P = list_size.size() * axis.size();
        r.stats.assign(P * POLAR_LS_N, 0);
        stat_rounds("list_stats", r.stats, POLAR_LS_N, POLAR_LS_ERR, POLAR_LS_RUN, max_runs, max_err, batch, [&](long t0, long T, const uint8_t *enabled) {
            return polar_mc_batch_list(_h, constellation, seed, (uint64_t)t0, T, 1, axis.data(), r.n_points, list_size.data(), r.n_L,
                                       enabled, r.stats.data());
        });
        r.bler.resize(P); r.miss_rate.resize(P); r.undetected_rate.resize(P); r.ml_bound.resize(P);
        for (size_t i = 0; i < P; ++i) {
            const uint64_t *s = &r.stats[i * POLAR_LS_N];
            const double run = s[POLAR_LS_RUN] ? (double)s[POLAR_LS_RUN] : 1.0;
            r.bler[i] = s[POLAR_LS_ERR] / run; r.miss_rate[i] = s[POLAR_LS_MISS] / run;
            r.undetected_rate[i] = s[POLAR_LS_UNDET] / run; r.ml_bound[i] = s[POLAR_LS_ML] / run;
        }
        return r;
    }
    // Adaptive list decoding (polar_decode_scl_llr_adaptive_batch; B codewords back to back): the list sizes of `schedule` (strictly
    // increasing, at most POLAR_AD_MAX_STAGES) in turn until the winner passes the CRC. out is decode_scl_llr's result at the list size
    // schedule[stage[b]]; crc_ok = 0 only at the last stage. The code needs a CRC.
    struct AdaptiveResult {
        long B = 0;
        int K = 0;
        std::vector<uint8_t> out;        // [B][K]
        std::vector<double> pm;          // [B]
        std::vector<uint8_t> stage;      // [B]
        std::vector<uint8_t> crc_ok;     // [B]
    };
    AdaptiveResult decode_scl_llr_adaptive(const std::vector<double> &llr, const std::vector<uint8_t> &schedule = {1, 4, 32}) {
        need(llr.size() % _block_length == 0, "decode_scl_llr_adaptive: size must be a multiple of block_length");
        AdaptiveResult r;
        r.B = (long)(llr.size() / _block_length); r.K = _info_length;
        r.out.resize((size_t)r.B * r.K); r.pm.resize((size_t)r.B); r.stage.resize((size_t)r.B); r.crc_ok.resize((size_t)r.B);
        check(polar_decode_scl_llr_adaptive_batch(_h, llr.data(), POLAR_LLR_F64, r.B, schedule.data(), (int)schedule.size(), r.out.data(),
                                                  r.pm.data(), r.stage.data(), r.crc_ok.data()));
        return r;
    }
    // The adaptive decoder over a sweep (polar_mc_batch_adaptive in rounds, stopped like list_stats). stats is
    // [point * (POLAR_AD_STAGE0 + n_stages) + POLAR_AD_*], stage_share [point * n_stages + stage]; mean_effort[point] = the mean over
    // the trials of schedule[0] + ... + schedule[stage] (a fixed list of L costs L).
    struct AdaptiveStats {
        int n_points = 0, n_stages = 0;
        std::vector<uint64_t> stats;
        std::vector<double> bler, undetected_rate, stage_share, mean_effort;
    };
    AdaptiveStats adaptive_stats(const std::vector<double> &axis, const std::vector<uint8_t> &schedule, long max_runs = 1000,
                                 long max_err = 100, uint64_t seed = 0, long batch = 0, int constellation = 0) {
        AdaptiveStats r;
        r.n_points = (int)axis.size(); r.n_stages = (int)schedule.size();
        const size_t P = axis.size(), C = (size_t)POLAR_AD_STAGE0 + schedule.size();
        r.stats.assign(P * C, 0);
        stat_rounds("adaptive_stats", r.stats, C, POLAR_AD_ERR, POLAR_AD_RUN, max_runs, max_err, batch, [&](long t0, long T, const uint8_t *enabled) {
            return polar_mc_batch_adaptive(_h, constellation, seed, (uint64_t)t0, T, 1, axis.data(), r.n_points, schedule.data(),
                                           r.n_stages, enabled, r.stats.data());
        });
        r.bler.resize(P); r.undetected_rate.resize(P); r.mean_effort.assign(P, 0.0); r.stage_share.resize(P * schedule.size());
        for (size_t i = 0; i < P; ++i) {
            const uint64_t *s = &r.stats[i * C];
            const double run = s[POLAR_AD_RUN] ? (double)s[POLAR_AD_RUN] : 1.0;
            r.bler[i] = s[POLAR_AD_ERR] / run; r.undetected_rate[i] = s[POLAR_AD_UNDET] / run;
            double cost = 0.0;
            for (size_t k = 0; k < schedule.size(); ++k) {
                cost += schedule[k];
                r.stage_share[i * schedule.size() + k] = s[POLAR_AD_STAGE0 + k] / run;
                r.mean_effort[i] += r.stage_share[i * schedule.size() + k] * cost;
            }
        }
        return r;
    }
    // SC-Flip (polar_decode_sc_flip_batch; B codewords back to back): one plain SC pass; while the word fails the CRC, whole re-decodes
    // with one decision inverted — the max_flips (0 .. POLAR_FLIP_MAX) unfrozen leaves of smallest |LLR| of the first pass, least
    // reliable first. n_dec = the passes taken, flip = the inverted position in decoding order (-1: none); cand / mag: the first pass's
    // candidates and their magnitudes (-1 / inf past K + crc). The code needs a CRC; block_length <= 4096.
    struct FlipResult {
        long B = 0;
        int K = 0, max_flips = 0;
        std::vector<uint8_t> out;        // [B][K]
        std::vector<uint8_t> crc_ok;     // [B]
        std::vector<uint8_t> n_dec;      // [B]
        std::vector<int32_t> flip;       // [B]
        std::vector<int32_t> cand;       // [B][max_flips]
        std::vector<double> mag;         // [B][max_flips]
    };
    FlipResult decode_sc_flip(const std::vector<double> &llr, int max_flips = 8) {
        need(llr.size() % _block_length == 0, "decode_sc_flip: size must be a multiple of block_length");
        need(max_flips >= 0 && max_flips <= POLAR_FLIP_MAX, "decode_sc_flip: max_flips out of range");
        FlipResult r;
        r.B = (long)(llr.size() / _block_length); r.K = _info_length; r.max_flips = max_flips;
        r.out.resize((size_t)r.B * r.K); r.crc_ok.resize((size_t)r.B); r.n_dec.resize((size_t)r.B); r.flip.resize((size_t)r.B);
        r.cand.resize((size_t)r.B * max_flips); r.mag.resize((size_t)r.B * max_flips);
        check(polar_decode_sc_flip_batch(_h, llr.data(), POLAR_LLR_F64, r.B, max_flips, r.out.data(), r.crc_ok.data(), r.n_dec.data(),
                                         r.flip.data(), r.cand.data(), r.mag.data()));
        return r;
    }
    // The SC-Flip decoder over a sweep (polar_mc_batch_flip in rounds, stopped like list_stats). stats is [point * POLAR_FL_N +
    // POLAR_FL_*]; mean_decodes[point] = DECODES / RUN: the SC passes a codeword took on average.
    struct FlipStats {
        int n_points = 0;
        std::vector<uint64_t> stats;
        std::vector<double> bler, undetected_rate, first_share, flipped_share, mean_decodes;
    };
    FlipStats flip_stats(const std::vector<double> &axis, int max_flips = 8, long max_runs = 1000, long max_err = 100, uint64_t seed = 0,
                         long batch = 0, int constellation = 0) {
        FlipStats r;
        r.n_points = (int)axis.size();
        const size_t P = axis.size(), C = POLAR_FL_N;
        r.stats.assign(P * C, 0);
        stat_rounds("flip_stats", r.stats, C, POLAR_FL_ERR, POLAR_FL_RUN, max_runs, max_err, batch, [&](long t0, long T, const uint8_t *enabled) {
            return polar_mc_batch_flip(_h, constellation, seed, (uint64_t)t0, T, 1, axis.data(), r.n_points, max_flips, enabled, r.stats.data());
        });
        r.bler.resize(P); r.undetected_rate.resize(P); r.first_share.resize(P); r.flipped_share.resize(P); r.mean_decodes.resize(P);
        for (size_t i = 0; i < P; ++i) {
            const uint64_t *s = &r.stats[i * C];
            const double run = s[POLAR_FL_RUN] ? (double)s[POLAR_FL_RUN] : 1.0;
            r.bler[i] = s[POLAR_FL_ERR] / run; r.undetected_rate[i] = s[POLAR_FL_UNDET] / run;
            r.first_share[i] = s[POLAR_FL_FIRST] / run; r.flipped_share[i] = s[POLAR_FL_FLIPPED] / run;
            r.mean_decodes[i] = s[POLAR_FL_DECODES] / run;
        }
        return r;
    }
    // SCAN soft-output decoding (polar_decode_scan_batch; B codewords back to back): the SC schedule with LLRs passed in both directions,
    // `iters` (1 .. POLAR_SCAN_MAX_ITERS) times; flags: POLAR_SCAN_MINSUM | POLAR_SCAN_EARLY_STOP (the latter needs a CRC). info_llr:
    // the LLRs of the info bits (out = info_llr < 0); ext: the extrinsic LLRs of the coded bits, indexed like the row (a posteriori:
    // llr + ext); n_iter: the iterations that ran. Rows must be finite; block_length <= 2048.
    struct ScanResult {
        long B = 0;
        int K = 0, N = 0;
        std::vector<uint8_t> out;        // [B][K]
        std::vector<double> info_llr;    // [B][K]
        std::vector<double> ext;         // [B][N]
        std::vector<uint8_t> crc_ok;     // [B]
        std::vector<uint8_t> n_iter;     // [B]
    };
    ScanResult decode_scan(const std::vector<double> &llr, int iters = 4, int flags = 0) {
        need(llr.size() % _block_length == 0, "decode_scan: size must be a multiple of block_length");
        need(iters >= 1 && iters <= POLAR_SCAN_MAX_ITERS, "decode_scan: iters out of range");
        ScanResult r;
        r.B = (long)(llr.size() / _block_length); r.K = _info_length; r.N = _block_length;
        r.out.resize((size_t)r.B * r.K); r.info_llr.resize((size_t)r.B * r.K); r.ext.resize((size_t)r.B * r.N);
        r.crc_ok.resize((size_t)r.B); r.n_iter.resize((size_t)r.B);
        check(polar_decode_scan_batch(_h, llr.data(), POLAR_LLR_F64, r.B, iters, flags, r.out.data(), r.info_llr.data(), r.ext.data(),
                                      r.crc_ok.data(), r.n_iter.data()));
        return r;
    }
    // The SCAN decoder over a sweep (polar_mc_batch_scan in rounds, stopped like list_stats). stats is [point * POLAR_SN_N +
    // POLAR_SN_*]; mean_iters[point] = ITERS / RUN: the iterations a codeword took on average.
    struct ScanStats {
        int n_points = 0;
        std::vector<uint64_t> stats;
        std::vector<double> bler, undetected_rate, mean_iters;
    };
    ScanStats scan_stats(const std::vector<double> &axis, int iters = 4, int flags = 0, long max_runs = 1000, long max_err = 100,
                         uint64_t seed = 0, long batch = 0, int constellation = 0) {
        ScanStats r;
        r.n_points = (int)axis.size();
        const size_t P = axis.size(), C = POLAR_SN_N;
        r.stats.assign(P * C, 0);
        stat_rounds("scan_stats", r.stats, C, POLAR_SN_ERR, POLAR_SN_RUN, max_runs, max_err, batch, [&](long t0, long T, const uint8_t *enabled) {
            return polar_mc_batch_scan(_h, constellation, seed, (uint64_t)t0, T, 1, axis.data(), r.n_points, iters, flags, enabled, r.stats.data());
        });
        r.bler.resize(P); r.undetected_rate.resize(P); r.mean_iters.resize(P);
        for (size_t i = 0; i < P; ++i) {
            const uint64_t *s = &r.stats[i * C];
            const double run = s[POLAR_SN_RUN] ? (double)s[POLAR_SN_RUN] : 1.0;
            r.bler[i] = s[POLAR_SN_ERR] / run; r.undetected_rate[i] = s[POLAR_SN_UNDET] / run; r.mean_iters[i] = s[POLAR_SN_ITERS] / run;
        }
        return r;
    }
    // Systematic coding (polar_encode_sys_batch, polar_sys_message_batch): B messages back to back -> B codewords that
    // carry them verbatim at systematic_positions(); `u_info` (optional) receives the precoded words, with encode(u_info) == coded.
    // systematic_message: the messages of B decoded u-domain words (any decoder's output); decode_scl_llr_systematic: both steps.
    std::vector<uint8_t> encode_systematic(const std::vector<uint8_t> &msg, std::vector<uint8_t> *u_info = nullptr) {
        need(msg.size() % _info_length == 0, "encode_systematic: size must be a multiple of info_length");
        const long B = (long)(msg.size() / _info_length);
        std::vector<uint8_t> coded((size_t)B * _block_length);
        if (u_info) u_info->assign(msg.size(), 0);
        if (B) check(polar_encode_sys_batch(_h, msg.data(), B, coded.data(), u_info ? u_info->data() : nullptr));
        return coded;
    }
    std::vector<uint8_t> systematic_message(const std::vector<uint8_t> &u_info) {
        need(u_info.size() % _info_length == 0, "systematic_message: size must be a multiple of info_length");
        std::vector<uint8_t> msg(u_info.size());
        if (!msg.empty()) check(polar_sys_message_batch(_h, u_info.data(), (long)(u_info.size() / _info_length), msg.data()));
        return msg;
    }
    std::vector<uint8_t> decode_scl_llr_systematic(const std::vector<double> &llr, uint16_t list_size) {
        return systematic_message(decode_scl_llr_batch(llr, list_size));
    }
    std::vector<uint16_t> systematic_positions() {
        std::vector<uint16_t> pos(_info_length);
        check(polar_get_sys_positions(_h, pos.data(), nullptr));
        return pos;
    }
    // Rate matching (polar_set_rate_match, polar_rate_match_batch, polar_decode_scl_llr_rm_batch): transmit position e
    // carries coded[sel[e]]; `known` (empty: none) marks the coded positions that are not sent and are 0 in every codeword. rate_match:
    // B codewords back to back -> B rows of sel.size() bits; decode_scl_llr_rm: B received rows of sel.size() LLRs -> the decoded info.
    void set_rate_match(const std::vector<uint16_t> &sel, const std::vector<uint8_t> &known = {}, double short_llr = 1000.0) {
        need(known.empty() || known.size() == _block_length, "set_rate_match: known must be empty or hold block_length entries");
        check(polar_set_rate_match(_h, sel.data(), (int)sel.size(), known.empty() ? nullptr : known.data(), short_llr));
        _rm_length = sel.size();
    }
    std::vector<uint8_t> rate_match(const std::vector<uint8_t> &coded) {
        need(_rm_length && coded.size() % _block_length == 0, "rate_match: no pattern set, or size not a multiple of block_length");
        const long B = (long)(coded.size() / _block_length);
        std::vector<uint8_t> tx((size_t)B * _rm_length);
        if (B) check(polar_rate_match_batch(_h, coded.data(), B, tx.data()));
        return tx;
    }
    std::vector<uint8_t> decode_scl_llr_rm(const std::vector<double> &rx, uint16_t list_size) {
        need(_rm_length && rx.size() % _rm_length == 0, "decode_scl_llr_rm: no pattern set, or size not a multiple of the transmit length");
        const long B = (long)(rx.size() / _rm_length);
        std::vector<uint8_t> out((size_t)B * _info_length);
        if (B) check(polar_decode_scl_llr_rm_batch(_h, rx.data(), POLAR_LLR_F64, B, list_size, out.data()));
        return out;
    }
    // Symbol-domain BICM receiver (PolarM/Constellation.m:123-144 in front of decode_scl_llr): received symbols, block_length /
    // n_bits per codeword, with noise variance n0 -> the bits decode_scl_llr gives on compute_llr_bicm's LLRs of them.
    // constellation_name as the reference's Constellation constructor takes it ("bpsk", "ask4-gray", ... "ask16-sp").
    // One codeword, or B codewords back to back (doubles or floats: a float is widened exactly on the device).
    std::vector<uint8_t> decode_bicm(const std::vector<double> &y, double n0, const std::string &constellation_name, uint16_t list_size) {
        const long B = bicm_rows(y.size(), constellation_name);
        std::vector<uint8_t> out((size_t)B * _info_length);
        check(polar_decode_bicm_batch(_h, constellation_id(constellation_name), y.data(), n0, B, list_size, out.data()));
        return out;
    }
    std::vector<uint8_t> decode_bicm(const std::vector<float> &y, double n0, const std::string &constellation_name, uint16_t list_size) {
        const long B = bicm_rows(y.size(), constellation_name);
        std::vector<uint8_t> out((size_t)B * _info_length);
        check(polar_decode_bicm_batch_f32(_h, constellation_id(constellation_name), y.data(), n0, B, list_size, out.data()));
        return out;
    }
    // POLAR_CONST_* of include/polar_synth.h by the reference's constellation name (Constellation.m:41-66)
    static int constellation_id(const std::string &name) {
        static const char *const names[] = {"", "ask4-gray", "ask8-gray", "ask16-gray", "bpsk", "ask4-sp", "ask8-sp", "ask16-sp"};
        for (int i = 1; i < 8; ++i)
            if (name == names[i]) return i;
        throw std::out_of_range("unknown constellation " + name);
    }

    // PolarCode.cpp:658: bler[list_index][ebno_index]; reference constants max_err=100, max_runs=1000
    // PolarCode.h:32-34. `devices` (optional): shard the trials of every round over these GPUs of the node
    // (polar_get_bler_quick_multi: one RCCL all-reduce of the counters per round); `ber` (optional): PolarM's
    // second output (PolarCode.m:781, 848), same layout as the result.
    std::vector<std::vector<double>> get_bler_quick(std::vector<double> ebno_vec, std::vector<uint8_t> list_size,
                                                    long max_runs = 1000, long max_err = 100, uint64_t seed = 1,
                                                    long batch = 0, std::vector<int> devices = {},
                                                    std::vector<std::vector<double>> *ber = nullptr, int constellation = 0) {
        // constellation: 0 = BPSK / Eb/N0 axis (PolarCode.cpp:744-753); POLAR_CONST_ASK{4,8,16}_GRAY (polar_synth.h) = the ASK
        // Gray + BICM sweep of PolarM/main_MC_CC_Comparison.m:44-119 with `ebno_vec` read as the SNR axis in dB
        std::vector<double> flat(ebno_vec.size() * list_size.size()), fber(flat.size());
        check(polar_get_bler_quick_multi_ex(_h, constellation, devices.empty() ? nullptr : devices.data(),
                                            devices.empty() ? 1 : (int)devices.size(), ebno_vec.data(), (int)ebno_vec.size(),
                                            list_size.data(), (int)list_size.size(), max_runs, max_err, seed, batch,   // batch 0: library rounds
                                            flat.data(), fber.data(), nullptr, nullptr, nullptr, nullptr));
        std::vector<std::vector<double>> bler(list_size.size(), std::vector<double>(ebno_vec.size()));
        if (ber) ber->assign(list_size.size(), std::vector<double>(ebno_vec.size()));
        for (size_t l = 0; l < list_size.size(); ++l)
            for (size_t e = 0; e < ebno_vec.size(); ++e) {
                bler[l][e] = flat[l * ebno_vec.size() + e];
                if (ber) (*ber)[l][e] = fber[l * ebno_vec.size() + e];
            }
        return bler;
    }
    // PolarM/PolarCode.m:198-255 ga_code_construction: in-place redesign by the Gaussian approximation on the GPU
    // (polar_ga_construction). `constellation` = POLAR_CONST_* of include/polar_synth.h (| POLAR_RX_MLC for the MLC receiver); capacities computed
    // by the library (integral for BPSK / MLC, 250 000-symbol polarized capacity of `seed` for multi-bit BICM). The frozen
    // set is the K+crc most reliable channels, the info order the stable descending order; the CRC matrix is kept.
    // Returns the BLER estimate (sum of qfunc(sqrt(c)/sqrt(2)) over the unfrozen channels); channels() holds the result.
    double ga_code_construction(double design_snr_db, int constellation = 4 /* POLAR_CONST_BPSK */, double phi_dx = 1e-5,
                                uint64_t seed = 1) {
        const size_t N = _block_length, k = (size_t)_info_length + _crc_size;
        std::vector<double> ch(N), pre(N);
        std::vector<uint16_t> order(N);
        check(polar_ga_construction(_n, constellation, &design_snr_db, 1, phi_dx, seed, nullptr, ch.data(), order.data(),
                                    pre.data()));
        std::vector<uint8_t> frozen(N, 1), crcm((size_t)_crc_size * _info_length);
        for (size_t i = 0; i < k; ++i) frozen[order[i]] = 0;
        if (_crc_size) check(polar_get_crc_matrix(_h, crcm.data()));
        polar_code_t *h = nullptr;
        const int rc = polar_create_explicit(_n, _info_length, _crc_size, frozen.data(), order.data(),
                                             _crc_size ? crcm.data() : nullptr, &h);
        check(rc);
        polar_destroy(_h);
        _h = h;
        _channels = ch;
        return pre[k - 1];
    }
    const std::vector<double> &channels() const { return _channels; }
    polar_code_t *handle() { return _h; }

private:
    static void check(int rc) {
        if (rc < 0) throw std::runtime_error(std::string("polar_amd: ") + polar_last_error());
    }
    static void need(bool ok, const char *msg) {
        if (!ok) throw std::out_of_range(msg);   // the reference throws out_of_range from .at()
    }
    // The rounds list_stats and adaptive_stats share: round(t0, T, enabled) adds the trials t0 .. t0 + T - 1 of the enabled cells to
    // stats ([cell * cols + column]). `batch` trials a round; 0: max(256, 2 max_err), then doubling up to 262144. A cell leaves once
    // ERR > max_err or RUN >= max_runs; no round goes past max_runs.
    template <typename Round>
    static void stat_rounds(const char *who, const std::vector<uint64_t> &stats, size_t cols, int err_col, int run_col, long max_runs, long max_err,
                            long batch, Round round) {
        need(max_runs >= 1 && batch >= 0, (std::string(who) + ": max_runs must be positive and batch non-negative").c_str());
        std::vector<uint8_t> enabled(stats.size() / cols);
        long done = 0, step = batch ? batch : (2 * max_err > 256 ? 2 * max_err : 256);
        while (done < max_runs) {
            bool any = false;
            for (size_t i = 0; i < enabled.size(); ++i) {
                enabled[i] = (long)stats[i * cols + err_col] <= max_err && (long)stats[i * cols + run_col] < max_runs;
                any = any || enabled[i];
            }
            if (!any) break;
            const long T = step < max_runs - done ? step : max_runs - done;
            check(round(done, T, enabled.data()));
            done += T;
            if (!batch) step = 2 * step < 262144 ? 2 * step : 262144;
        }
    }
    long bicm_rows(size_t n_sym, const std::string &name) const {
        const int id = constellation_id(name);
        const size_t M = _block_length / (size_t)(id == 4 ? 1 : id == 1 || id == 5 ? 2 : id == 2 || id == 6 ? 3 : 4);
        need(M > 0 && n_sym % M == 0, "decode_bicm: size must be a multiple of block_length / n_bits");
        return (long)(n_sym / M);
    }
    polar_code_t *_h = nullptr;
    uint8_t _n;
    uint16_t _info_length, _block_length = 0, _crc_size;
    size_t _rm_length = 0;           // transmit positions of the rate-matching pattern set (0: none)
    std::vector<double> _channels;
};

#endif
