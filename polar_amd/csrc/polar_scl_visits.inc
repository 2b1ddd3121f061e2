// polar_scl_visits.inc — BODY FRAGMENT of scl_decode_llr_kernel (polar_kernels.hip), included inside its leaf loop:
// recursivelyCalcLLR (PolarCode.cpp:422-455) for the leaf `phi` — the visits of the layers lam_top .. lam_stop: table build
// (list of 32), fused two- and four-layer passes over the HBM-resident layers, the LDS-resident bottom of the tree, the generic
// one-layer visit; the one-codeword-per-wave (LAT) form. Not a translation unit of its own: it uses the kernel's locals.
            // ---------------- recursivelyCalcLLR(n, phi): PolarCode.cpp:422-455 ----------------
            const int lam_top = (phi == phi_start && forced_top) ? forced_top : (phi ? (n - __builtin_ctz((unsigned)phi)) : 1);
            double leaf = 0.0;
            if constexpr (LAT) {
                // ---- the one-codeword-per-wave form (see the template's comment): the elements of a layer are spread over the 64 / GS
                // lanes of each path. Round 6: a lone wave pays 4 cycles for EVERY instruction it issues, scalar or vector, 20 for a
                // taken branch and ~ 50-60 for an LDS round trip (tools/lone_wave_microbench.hip), so the two lowest layers — three
                // quarters of all visits — are straight-line code on registers outside the layer loop.
                // (ED) The lanes of a path that is NOT active run the visits below all the same, on whatever their slot pointers lead to —
                // at a layer this codeword has not written in that slot yet, the values the wave's PREVIOUS codeword left there. Nothing
                // they compute is stored, but their guard distance would be kept: a codeword that follows one with an f-node in the
                // window would be flagged with it. Only what a living path evaluates counts.
                [[maybe_unused]] const double gacc_in = gacc;
                const bool bottom_regs = n >= 3;
                const int lam_hi = bottom_regs ? (lam_stop < n - 2 ? lam_stop : n - 2) : lam_stop;
                for (int lam = lam_top; lam <= lam_hi; ++lam) {
                    const int sh_ = n - lam, S_ = 1 << sh_, e_ = lane_k / GS;
                    const bool odd_ = (phi >> sh_) & 1;
                    const int pin_ = (lam > 1) ? pL.get(sh_ + 1) : 0;
                    const double *srcp = (lam > 1) ? lat_a + (size_t)(2 * S_ - 1) * GS + pin_ : lat_ch;
                    const int sstr = (lam > 1) ? GS : 1;
                    double *dstp = lat_a + (size_t)(S_ - 1) * GS + lig;
                    const uint32_t *cwp_ = (odd_ && S_ > 32) ? g_cl + (size_t)(S_ / 32 - 2) * CST + pC.get(sh_) : nullptr;
                    auto one = [&](int j, double a_, double b_) -> double {
                        if (!odd_) return FN(a_, b_);
                        if (S_ <= 32) return GN(a_, b_, (uint32_t)(clsmall >> S_), j);
                        return GN(a_, b_, cwp_[(size_t)(j >> 5) * CST], j & 31);
                    };
                    if (S_ == 1) {
                        // (block lengths below 8) the leaf's own node: every lane of the path evaluates it from the same two operands
                        // (a broadcast read) — not stored and read back — and keeps them for the right leaf of the pair
                        if (!(odd_ && lat_yv)) { lat_y0 = srcp[0]; lat_y1 = srcp[sstr]; }
                        lat_yv = !odd_;
                        leaf = one(0, lat_y0, lat_y1);
                        PROF(4)
                        continue;
                    }
                    if (S_ >= 4 * EL) {
                        for (int j0 = e_; j0 < S_; j0 += 4 * EL) {
                            double a_[4], b_[4], r_[4];
#pragma unroll
                            for (int k = 0; k < 4; ++k) { a_[k] = srcp[(size_t)(j0 + k * EL) * sstr]; b_[k] = srcp[(size_t)(j0 + k * EL + S_) * sstr]; }
#pragma unroll
                            for (int k = 0; k < 4; ++k) r_[k] = one(j0 + k * EL, a_[k], b_[k]);
                            if (active) {
#pragma unroll
                                for (int k = 0; k < 4; ++k) dstp[(size_t)(j0 + k * EL) * GS] = r_[k];
                            }
                        }
                    } else {
                        for (int j = e_; j < (S_ > EL ? S_ : EL); j += EL) {
                            const bool in_ = j < S_;
                            const double a_ = srcp[(size_t)(in_ ? j : 0) * sstr], b_ = srcp[(size_t)((in_ ? j : 0) + S_) * sstr];
                            const double r_ = one(in_ ? j : 0, a_, b_);
                            if (active && in_) dstp[(size_t)j * GS] = r_;
                        }
                    }
                    if (active) pL.set(sh_, lig);
                    wave_mem_fence();
                    PROF(S_ >= EL ? (odd_ ? 1 : 2) : (S_ >= 4 ? 3 : 4))
                }
                if (bottom_regs && lam_stop == n) {
                    // The two lowest layers in registers. Every lane of a path reads the FOUR values of its layer of size 4 once per
                    // quad of leaves (a broadcast read, at the quad's first leaf, right after that layer's own visit) and evaluates the
                    // nodes below — two of the layer of size 2, the leaf's — itself: same operands, same arithmetic, same values as
                    // the stored layers held. A clone in a leaf step copies lat_x / lat_y from its source lane like the rest of the
                    // path's state (polar_scl_leaf.inc).
                    if ((phi & 1) == 0) {
                        if ((phi & 2) == 0) {
                            const double *xs = lat_a + (size_t)3 * GS + lig;          // (its own slot: the visit above has just written it)
#pragma unroll
                            for (int k = 0; k < 4; ++k) lat_x[k] = xs[(size_t)k * GS];
                            FN2(lat_x[0], lat_x[2], lat_x[1], lat_x[3], lat_y0, lat_y1);
                        } else {
                            const uint32_t cb_ = (uint32_t)(clsmall >> 2);
                            lat_y0 = GN(lat_x[0], lat_x[2], cb_, 0); lat_y1 = GN(lat_x[1], lat_x[3], cb_, 1);
                        }
                        leaf = FN(lat_y0, lat_y1);
                    } else {
                        leaf = GN(lat_y0, lat_y1, (uint32_t)(clsmall >> 1), 0);
                    }
                    PROF(4)
                }
                if constexpr (ED) { if (!active) gacc = gacc_in; }
            } else
            for (int lam = lam_top; lam <= lam_stop; ++lam) {
                if (POLAR_UNLIKELY2(tbl && lam <= 2 && phi >= S2)) {
                    // phi = N/4, N/2, 3N/4: the visits of layers 1 and 2 are replaced by the table build
                    const int kind = phi / S2;                      // 1: h (g of the shared layer 1), 2: f, 3: g
                    LANE_CTX
                    double *Xc = tab_w + (size_t)(lane / GS) * (size_t)(3 * N), *T2c = Xc + N;
                    if (valid) {                                    // all lanes of the codeword, whatever their path's state
                        if (kind == 1) {
                            const double *x1f = p.pre + cw_of_lane(lane) * (size_t)(N - p.prefix_q + 1) + 1;     // layer 1, first half (prefix kernel)
                            for (int j = lig; j < S2; j += GS) {
                                const double a = x1f[j], b = x1f[j + S2];
                                T2c[8 * j + 0] = g_node_e(a, b, 0u, tb);
                                T2c[8 * j + 1] = g_node_e(a, b, 0x80000000u, tb);
                            }
                        } else {
                            if (kind == 2) {
                                const double *chr = ch_row<CH_N16>(p, cw_of_lane(lane), N);
                                for (int e = lig; e < S1; e += GS) {
                                    const unsigned i0 = __brev((unsigned)e) >> (32 - n);
                                    const double a = CH(chr, i0), b = CH(chr, i0 + 1);
                                    Xc[2 * e + 0] = g_node_e(a, b, 0u, tb);
                                    Xc[2 * e + 1] = g_node_e(a, b, 0x80000000u, tb);
                                }
                                wave_mem_fence();
                            }
                            for (int j = lig; j < S2; j += GS) {
                                const double a0 = Xc[2 * j], a1 = Xc[2 * j + 1], b0 = Xc[2 * (j + S2)], b1 = Xc[2 * (j + S2) + 1];
                                if (kind == 2) {
                                    T2c[8 * j + 0] = f_node_e(a0, b0, guard); T2c[8 * j + 1] = f_node_e(a1, b0, guard);
                                    T2c[8 * j + 2] = f_node_e(a0, b1, guard); T2c[8 * j + 3] = f_node_e(a1, b1, guard);
                                } else {
#pragma unroll
                                    for (int v = 0; v < 8; ++v)
                                        T2c[8 * j + v] = g_node_e((v & 1) ? a1 : a0, (v & 2) ? b1 : b0, (unsigned)(v >> 2) << 31, tb);
                                }
                            }
                        }
                    }
                    // the path's variant nibbles V[e] = u1[e] | u1[e + N/4] << 1 | u2[e] << 2 (kind 1: u2[e] only), 8 per word
                    // (packing them per consumer pass instead — two words per pass — costs more in the build than the
                    // visit saves: -5 %)
                    if (active) {
                        const uint32_t *c1p = g_cl + (size_t)(S1 / 32 - 2) * 64 + gbase + pC.get(n - 1);
                        const uint32_t *c2p = g_cl + (size_t)(S2 / 32 - 2) * 64 + gbase + pC.get(n - 2);
                        auto spread = [](uint32_t x) {               // bit i of the low byte -> bit 4i
                            uint32_t t = (x | (x << 12)) & 0x000F000Fu;
                            t = (t | (t << 6)) & 0x03030303u;
                            return (t | (t << 3)) & 0x11111111u;
                        };
                        for (int w32 = 0; w32 < S2 / 32; ++w32) {
                            const uint32_t ua = (kind >= 2) ? c1p[(size_t)w32 * 64] : 0u, ub = (kind >= 2) ? c1p[(size_t)(w32 + S2 / 32) * 64] : 0u;
                            const uint32_t uc = (kind != 2) ? c2p[(size_t)w32 * 64] : 0u;
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                uint32_t vw;
                                if (kind == 1) vw = spread((uc >> (8 * q)) & 0xFFu);
                                else vw = spread((ua >> (8 * q)) & 0xFFu) | (spread((ub >> (8 * q)) & 0xFFu) << 1) | (spread((uc >> (8 * q)) & 0xFFu) << 2);
                                g_v[(size_t)(4 * w32 + q) * 64 + lane] = vw;
                            }
                        }
                        pC.set(15, lig);                             // slot of this path's V words
                    }
                    wave_mem_fence();
                    lam = 2;
                    continue;                                        // next: layer 3 with the table as its source
                }
                const int sh = n - lam;
                const int S = 1 << sh;
                const bool odd = (phi >> sh) & 1;
                // ---- fused visit of two consecutive layers (lam: size S, op f/g; lam+1: size S/2, always
                // f right after): the values of layer lam are written (the later g-visit of lam+1 needs
                // them) but NOT re-read from HBM for the f-visit of lam+1. Only when the source of lam
                // is HBM-resident (channel LLRs or a scratch layer).
#ifdef POLAR_SLOTHIST
                // Measurement build (tools/slot_histogram.py; round-3 verdict item 2): for every visit whose SOURCE layer is
                // HBM-resident, how many DISTINCT source slots the active paths of a codeword read (pL.get(sh + 1)) — per
                // visit kind (f / g) and layer size. An f-visit whose source slots coincide would compute and store identical
                // rows. hist[kind][sh][distinct] += 1, plus sum of active paths and of paths reading their OWN slot.
                if (GS == 32 && lam > 1 && 2 * S > SL && p.pm_out) {
                    LANE_CTX
                    const bool in_pre_ = p.prefix_q > 0 && 2 * S >= p.prefix_q && phi < 2 * S;
                    const bool tab_ = tbl && lam == 3 && phi >= S2;
                    if (!in_pre_ && !tab_) {
                        const int pin_ = pL.get(sh + 1);
                        int d0 = 0, d1 = 0;
                        for (int s_ = 0; s_ < 32; ++s_) {
                            const u64 m_ = __ballot(active && pin_ == s_);
                            d0 += (m_ & 0xFFFFFFFFull) != 0; d1 += (m_ >> 32) != 0;
                        }
                        const u64 own_ = __ballot(active && pin_ == lig);
                        u64 *hb = reinterpret_cast<u64 *>(p.pm_out) + 64 + (size_t)((odd ? 1 : 0) * 12 + sh) * 40;
                        if (lane == 0) {
                            if (actw & 0xFFFFFFFFull) { atomicAdd(hb + d0, 1ull); atomicAdd(hb + 34, (u64)__popcll(actw & 0xFFFFFFFFull)); atomicAdd(hb + 35, (u64)__popcll(own_ & 0xFFFFFFFFull)); }
                            if (actw >> 32) { atomicAdd(hb + d1, 1ull); atomicAdd(hb + 34, (u64)__popcll(actw >> 32)); atomicAdd(hb + 35, (u64)__popcll(own_ >> 32)); }
                        }
                    }
                }
#endif
                if (!PIPE && S >= 8 && 2 * S > SL && lam + 1 <= lam_stop && ((phi >> (sh - 1)) & 1) == 0) {   // (lam+1 is an f-visit)
                    const int H = S / 2;
#ifdef POLAR_SADDR
                    // (not from the prefix buffer, whose rows are per codeword: once per codeword, left to the two-layer body)
                    const bool deep = (lam + 3 <= lam_stop) && (phi & (S - 1)) == 0 && !(lam > 1 && p.prefix_q > 0 && 2 * S >= p.prefix_q && phi < 2 * S);
#else
                    const bool deep = (lam + 3 <= lam_stop) && (phi & (S - 1)) == 0;        // four layers at once (else two)
#endif
                    if (active) {
                        LANE_CTX
                        const bool in_is_ch = (lam == 1);
                        const bool in_pre = !in_is_ch && p.prefix_q > 0 && 2 * S >= p.prefix_q && phi < 2 * S;
                        // (active lanes are valid ones: codeword g0 + lane / GS)
                        const double *in0 = in_is_ch ? ch_row<CH_N16>(p, cw_of_lane(lane), N) : nullptr;
                        const double *pre_cw = in_pre ? p.pre + cw_of_lane(lane) * (size_t)(N - p.prefix_q + 1) : nullptr;
                        const int pin = (in_is_ch || in_pre) ? 0 : pL.get(sh + 1);
                        const size_t istr = in_pre ? 1 : 64;      // prefix layers are contiguous per codeword
                        const double *gin = in_is_ch ? nullptr : (in_pre ? pre_cw + 1 + (size_t)(N - 4 * S)
                                                                         : g_llr + (size_t)(2 * S - 2 * SL) * 64 + gbase + pin);
                        uint32_t cb0 = 0, cb1 = 0;          // partial-sum bits for elements j.. and j+H..
                        const uint32_t *cwp = nullptr;
                        if (odd) {
                            if (S <= 32) { cb0 = (uint32_t)(clsmall >> S); cb1 = cb0 >> H; }
                            else cwp = g_cl + (size_t)(S / 32 - 2) * 64 + gbase + pC.get(sh);
                        }
                        // the body is instantiated once per address-space combination of its outputs: a pointer
                        // that may be LDS or global degrades every access to a FLAT instruction, which waits on
                        // vmcnt AND lgkmcnt (i.e. for every outstanding HBM store) before a dependent use
                        auto fused_body = [&](const double *inp, double *out0, double *out1) {
                            for (int j = 0; j < H; j += FU) {
                                double a0[FU], b0[FU], a1[FU], b1[FU];
                                if (in_is_ch) {
#pragma unroll
                                    for (int k = 0; k < FU; ++k) {
                                        unsigned i0 = __brev((unsigned)(j + k)) >> (32 - n);
                                        unsigned i1 = __brev((unsigned)(j + k + H)) >> (32 - n);
                                        a0[k] = CH(in0, i0); b0[k] = CH(in0, i0 + 1);
                                        a1[k] = CH(in0, i1); b1[k] = CH(in0, i1 + 1);
                                    }
                                } else {
#pragma unroll
                                    for (int k = 0; k < FU; ++k) {
                                        a0[k] = inp[(size_t)(j + k) * istr];
                                        b0[k] = inp[(size_t)(j + k + S) * istr];
                                        a1[k] = inp[(size_t)(j + k + H) * istr];
                                        b1[k] = inp[(size_t)(j + k + H + S) * istr];
                                    }
                                }
                                if (odd && S > 32 && (j & 31) == 0) {
                                    cb0 = cwp[(size_t)(j >> 5) * 64];
                                    cb1 = (H >= 32) ? cwp[(size_t)((j + H) >> 5) * 64] : (cb0 >> H);
                                }
                                // element by element: (x0, x1) of layer lam -> stored -> y of layer lam+1 -> stored
#pragma unroll
                                for (int k = 0; k < FU; ++k) {
                                    double x0, x1;
                                    if (odd) {
                                        const int bi = (S > 32) ? ((j + k) & 31) : (j + k);
                                        x0 = GN(a0[k], b0[k], cb0, bi);
                                        x1 = GN(a1[k], b1[k], cb1, bi);
                                    } else {
                                        x0 = FN(a0[k], b0[k]);
                                        x1 = FN(a1[k], b1[k]);
                                    }
                                    out0[(size_t)(j + k) * 64] = x0;
                                    out0[(size_t)(j + k + H) * 64] = x1;
                                    out1[(size_t)(j + k) * 64] = FN(x0, x1);
                                }
                            }
                        };
                        // ---- four layers in one pass (lam .. lam+3, sizes S, S/2, S/4, S/8): element j of the lowest
                        // one is a 3-stage f-tree over the eight elements j + m*S/8 of layer lam, so none of the three
                        // intermediate layers is re-read from HBM by the f-visit below it (they are still written:
                        // the later g-visits need them). 16 loads in flight per pass, as the two-layer body.
                        // (measured and dropped: not storing layer 1's second half — the largest array — and re-deriving it
                        // from the channel values at its only later reader, the g-visit of layer 2 at phi = 3N/4: -9 % HBM
                        // bytes, but -1.7 % throughput; the re-derivation pass itself is slower than the traffic it saves)
#if POLAR_HEAD == 2
                        // (a walk that starts INSIDE the second quarter has no table of the h values — the head kept layer 2 as an
                        // ordinary layer, handed over in the record — and takes the tables up with the build at N/2; a walk that
                        // starts AT N/4 runs that build itself, like one that starts before it)
                        const bool tsrc = tbl && lam == 3 && phi >= S2 && (phi >= S1 || p.head_phi <= S2);
#else
                        const bool tsrc = tbl && lam == 3 && phi >= S2;       // inputs come from the layer-2 table
#endif
                        // GMM: bit k set = o_k is HBM-resident and passed as the UNIFORM base of its rows (the lane offset is added as a
                        // 32-bit register offset: global_load/store with an SGPR base, no 64-bit VALU add per access)
                        auto fused4 = [&](const double *inp, double *o0, double *o1, double *o2, double *o3, auto NTT, auto TSS, auto GMM) {
                            constexpr bool TS = decltype(TSS)::value;
                            constexpr int GM = decltype(GMM)::value;
                            const uint32_t lb = (uint32_t)lane * 8u;
                            const uint32_t lin = (uint32_t)(gbase + pin) * 8u;
                            const char *inu = reinterpret_cast<const char *>(g_llr + (size_t)(2 * S - 2 * SL) * 64);      // source rows (uniform)
                            auto st = [&](double *o, auto gbit, auto ntbit, size_t row, double val) {
                                constexpr bool G_ = decltype(gbit)::value, N_ = decltype(ntbit)::value;
                                double *q_ = G_ ? reinterpret_cast<double *>(reinterpret_cast<char *>(o) + row * 512 + lb) : o + row * 64;
                                if (N_) __builtin_nontemporal_store(val, q_); else *q_ = val;
                            };
                            // streaming (non-temporal) accesses for the layers of size >= 64 (bit 0: input, 1: o0, 2: o1): they
                            // are written once and read once or twice much later; the layers of size 16 and 32 stay cacheable
                            // (measured +1.7 %)
                            constexpr int NT = decltype(NTT)::value;
                            const int E = S >> 3;
                            uint32_t cw8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                            if (odd && S <= 32) cw8[0] = (uint32_t)(clsmall >> S);
                            double a[8], b[8], v[8];
                            const double *T2c = TS ? tab_w + (size_t)(lane / GS) * (size_t)(3 * N) + N : nullptr;
                            const uint32_t *vp = TS ? g_v + gbase + pC.get(15) : nullptr;
                            auto load8 = [&](int j) {
                                if (TS) {
#pragma unroll
                                    for (int m = 0; m < 8; ++m) {
                                        const int e0 = j + m * E, e1 = e0 + S;            // elements of layer 2
                                        const uint32_t w0 = vp[(size_t)(e0 >> 3) * 64], w1 = vp[(size_t)(e1 >> 3) * 64];
                                        a[m] = T2c[8 * e0 + ((w0 >> (4 * (e0 & 7))) & 7u)];
                                        b[m] = T2c[8 * e1 + ((w1 >> (4 * (e1 & 7))) & 7u)];
                                    }
                                } else if (in_is_ch) {
#pragma unroll
                                    for (int m = 0; m < 8; ++m) {
                                        const unsigned i0 = __brev((unsigned)(j + m * E)) >> (32 - n);
                                        a[m] = CH(in0, i0); b[m] = CH(in0, i0 + 1);
                                    }
                                } else {
                                    const int jj = j;
#pragma unroll
                                    for (int m = 0; m < 8; ++m) {
#ifdef POLAR_SADDR
                                        // (never the prefix buffer here: `deep` excludes it)
                                        const double *pa = reinterpret_cast<const double *>(inu + (size_t)(jj + m * E) * 512 + lin);
                                        const double *pb = reinterpret_cast<const double *>(inu + (size_t)(jj + m * E + S) * 512 + lin);
                                        if (NT & 1) { a[m] = __builtin_nontemporal_load(pa); b[m] = __builtin_nontemporal_load(pb); }
                                        else { a[m] = *pa; b[m] = *pb; }
#else
                                        if (NT & 1) { a[m] = __builtin_nontemporal_load(inp + (size_t)(jj + m * E) * istr); b[m] = __builtin_nontemporal_load(inp + (size_t)(jj + m * E + S) * istr); }
                                        else { a[m] = inp[(size_t)(jj + m * E) * istr]; b[m] = inp[(size_t)(jj + m * E + S) * istr]; }
#endif
                                    }
                                }
                            };
                            // (measured and dropped, round 3: an L2 prefetch of the NEXT pass's 16 source rows by ONE scattered
                            // global_load_dword touching their 64 lines — no VGPRs, no wait: -1.5 %; the kernel is on the bandwidth
                            // ceiling of its access pattern, asking earlier gains nothing)
                            for (int j = 0; j < E; ++j) {
                                load8(j);
                                if (odd && S > 32 && (j & 31) == 0) {
#pragma unroll
                                    for (int m = 0; m < 8; ++m) cw8[m] = cwp[(size_t)((j + m * E) >> 5) * 64];
                                }
#pragma unroll
                                for (int m = 0; m < 8; ++m) {
                                    if (odd) v[m] = (S > 32) ? GN(a[m], b[m], cw8[m], (j + m * E) & 31) : GN(a[m], b[m], cw8[0], j + m * E);
                                    else v[m] = FN(a[m], b[m]);
                                }
                                // (issuing the next pass's loads here, ahead of the 15 stores, was measured: -15 % — the
                                // double-buffered inputs do not fit the 128-VGPR budget)
                                const int js = j;
                                typedef std::integral_constant<bool, (GM & 1) != 0> G0; typedef std::integral_constant<bool, (GM & 2) != 0> G1;
                                typedef std::integral_constant<bool, (GM & 4) != 0> G2; typedef std::integral_constant<bool, (GM & 8) != 0> G3;
                                typedef std::integral_constant<bool, (NT & 2) != 0> N0; typedef std::integral_constant<bool, (NT & 4) != 0> N1;
                                typedef std::integral_constant<bool, (NT & 8) != 0> N2; typedef std::integral_constant<bool, false> N3;
#pragma unroll
                                for (int m = 0; m < 8; ++m) st(o0, G0{}, N0{}, (size_t)(js + m * E), v[m]);
#pragma unroll
                                for (int m = 0; m < 4; ++m) { v[m] = FN(v[m], v[m + 4]); st(o1, G1{}, N1{}, (size_t)(js + m * E), v[m]); }
#pragma unroll
                                for (int m = 0; m < 2; ++m) { v[m] = FN(v[m], v[m + 2]); st(o2, G2{}, N2{}, (size_t)(js + m * E), v[m]); }
                                v[0] = FN(v[0], v[1]);
                                st(o3, G3{}, N3{}, (size_t)j, v[0]);
                                leaf = v[0];            // (the leaf value when S/8 == 1)
                            }
                        };
#define POLAR_GROW(T) (g_llr + (size_t)((T) - 2 * SL) * 64 + lane)
#define POLAR_LROW(T) (lds_llr + (size_t)((T) - 1) * 64 + lane)
                        if (deep) {
                            const int Q = S / 4, E8 = S / 8;
                            // (also streaming the layer of size 32, so that only the layer of size 16 competes for the L2: -0.5 %)
#define POLAR_NTM(x) std::integral_constant<int, (x)>{}
                            typedef std::integral_constant<bool, false> TS0;
#ifdef POLAR_SADDR
#define POLAR_GOUT(T) (g_llr + (size_t)((T) - 2 * SL) * 64)
#define POLAR_GMK(x) std::integral_constant<int, (x)>{}
#else
#define POLAR_GOUT(T) POLAR_GROW(T)
#define POLAR_GMK(x) std::integral_constant<int, 0>{}
#endif
                            if (tsrc) fused4(gin, POLAR_GOUT(S), POLAR_GOUT(H), POLAR_GOUT(Q), POLAR_GOUT(E8), POLAR_NTM(6), std::integral_constant<bool, true>{}, POLAR_GMK(15));
                            else if (E8 > SL) fused4(gin, POLAR_GOUT(S), POLAR_GOUT(H), POLAR_GOUT(Q), POLAR_GOUT(E8), POLAR_NTM(7), TS0{}, POLAR_GMK(15));      // S >= 128
                            else if (Q > SL) fused4(gin, POLAR_GOUT(S), POLAR_GOUT(H), POLAR_GOUT(Q), POLAR_LROW(E8), POLAR_NTM(3), TS0{}, POLAR_GMK(7));   // S = 64
                            else if (H > SL) fused4(gin, POLAR_GOUT(S), POLAR_GOUT(H), POLAR_LROW(Q), POLAR_LROW(E8), POLAR_NTM(1), TS0{}, POLAR_GMK(3));   // S = 32: input 64
                            else if (S > SL) fused4(gin, POLAR_GOUT(S), POLAR_LROW(H), POLAR_LROW(Q), POLAR_LROW(E8), POLAR_NTM(0), TS0{}, POLAR_GMK(1));                 // S = 16: input 32
                            else fused4(gin, POLAR_LROW(S), POLAR_LROW(H), POLAR_LROW(Q), POLAR_LROW(E8), std::integral_constant<int, 0>{}, TS0{}, POLAR_GMK(0));        // S = 8: input 16
#undef POLAR_GOUT
#undef POLAR_GMK
#undef POLAR_NTM
                            pL.set(sh - 2, lig);
                            pL.set(sh - 3, lig);
                        }
                        else if (S <= SL) fused_body(gin, POLAR_LROW(S), POLAR_LROW(H));
                        else if (H <= SL) fused_body(gin, POLAR_GROW(S), POLAR_LROW(H));
                        else fused_body(gin, POLAR_GROW(S), POLAR_GROW(H));
#undef POLAR_GROW
#undef POLAR_LROW
                        pL.set(sh, lig);
                        pL.set(sh - 1, lig);
                    }
                    wave_mem_fence();
                    PROF(odd ? 1 : 2)
#ifdef POLAR_SLOTHIST
                    if (GS == 32 && p.pm_out && lane == 0 && actw) {      // f-visits of this pass fed from registers (the path's own values)
                        u64 *hb = reinterpret_cast<u64 *>(p.pm_out) + 64 + (size_t)24 * 40;
                        for (int d_ = 1; d_ <= (deep ? 3 : 1); ++d_) if ((S >> d_) > SL) atomicAdd(hb + (sh - d_), 1ull);
                    }
#endif
                    lam += deep ? 3 : 1;          // layers lam+1 (.. lam+3) are done
                    continue;
                }
                // ---- both layers in LDS (the bottom of the tree, visited at almost every leaf): plain ds_read /
                // ds_write on provably-LDS pointers, all inputs of the visit loaded before the first f
                if (lam > 1 && 2 * S <= SL) {
                    // the f-visits of the layers below follow immediately (phi is a multiple of S): they are taken
                    // from registers in the same pass — `below` more layers, down to the leaf or the rate-0 block
                    // (not at the resume point of the all-frozen prefix, where phi is not a multiple of S)
                    const int below = ((phi & (S - 1)) == 0) ? lam_stop - lam : 0;
                    if (active) {
                        LANE_CTX
                        const double *li = lds_llr + (size_t)(2 * S - 1) * 64 + gbase + pL.get(sh + 1);
                        double *lo = lds_llr + (size_t)(S - 1) * 64 + lane;
                        const uint32_t cb = odd ? (uint32_t)(clsmall >> S) : 0u;
                        auto small = [&](auto SS) {
                            constexpr int S_ = decltype(SS)::value;
                            double a[S_], b[S_], r[S_];
#pragma unroll
                            for (int j = 0; j < S_; ++j) { a[j] = li[(size_t)j * 64]; b[j] = li[(size_t)(j + S_) * 64]; }
#pragma unroll
                            for (int j = 0; j < S_; ++j) r[j] = odd ? GN(a[j], b[j], cb, j) : FN(a[j], b[j]);
                            // (the layer of size 1 — the leaf value — is consumed from the register: nobody reads it back)
                            if (S_ > 1 || !POLAR_SKIP_L1) {
#pragma unroll
                                for (int j = 0; j < S_; ++j) lo[(size_t)j * 64] = r[j];
                            }
                            // layer of size T = S_ >> d from the one above (registers), stored for its later g-visit
                            auto down = [&](auto TT) {
                                constexpr int T = decltype(TT)::value;
                                double *lt = lds_llr + (size_t)(T - 1) * 64 + lane;
#pragma unroll
                                for (int j = 0; j < T; ++j) { r[j] = FN(r[j], r[j + T]); if (T > 1 || !POLAR_SKIP_L1) lt[(size_t)j * 64] = r[j]; }
                            };
                            if constexpr (S_ >= 2) { if (below >= 1) down(std::integral_constant<int, S_ / 2>{}); }
                            if constexpr (S_ >= 4) { if (below >= 2) down(std::integral_constant<int, S_ / 4>{}); }
                            if constexpr (S_ >= 8) { if (below >= 3) down(std::integral_constant<int, S_ / 8>{}); }
                            if constexpr (S_ >= 16) { if (below >= 4) down(std::integral_constant<int, S_ / 16>{}); }
                            leaf = r[0];            // (the leaf LLR when the chain reached the layer of size 1)
                        };
                        if (S == 1) small(std::integral_constant<int, 1>{});
                        else if (S == 2) small(std::integral_constant<int, 2>{});
                        else if (S == 4) small(std::integral_constant<int, 4>{});
                        else if (S == 8) small(std::integral_constant<int, 8>{});
                        else small(std::integral_constant<int, 16>{});      // (lds_log = 5)
                        for (int d = 0; d <= below; ++d) if (sh - d > 0 || !POLAR_SKIP_L1) pL.set(sh - d, lig);
                    }
                    wave_mem_fence();
                    PROF(S >= 4 ? 3 : 4)
                    lam += below;
                    continue;
                }
                if (active) {
                    LANE_CTX
                    // input layer lam-1 (size 2S): 0 = channel LLRs, else scratch/LDS slot
                    const int pin = (lam > 1) ? pL.get(sh + 1) : 0;
                    const double *inp;   // element j at inp[j*istride]
                    size_t istride;
                    const bool in_is_ch = (lam == 1);
                    const bool in_pre = !in_is_ch && p.prefix_q > 0 && 2 * S >= p.prefix_q && phi < 2 * S;
                    const double *in0 = in_is_ch ? ch_row<CH_N16>(p, cw_of_lane(lane), N) : nullptr;
                    const double *pre_cw = in_pre ? p.pre + cw_of_lane(lane) * (size_t)(N - p.prefix_q + 1) : nullptr;
                    constexpr bool in_lds = false;          // (LDS inputs were handled above)
                    istride = 64;
                    if (in_pre) { inp = pre_cw + 1 + (size_t)(N - 4 * S); istride = 1; }
                    else if (!in_is_ch) inp = g_llr + (size_t)(2 * S - 2 * SL) * 64 + gbase + pin;
                    else inp = nullptr;
                    const bool out_lds = (S <= SL);
                    auto generic_body = [&](double *outp) {
                    // partial sums for g (column 0 of C_lam)
                    uint32_t cbits = 0;
                    const uint32_t *cwp = nullptr;
                    if (odd) {
                        if (S <= 32) cbits = (uint32_t)(clsmall >> S);
                        else cwp = g_cl + (size_t)(S / 32 - 2) * 64 + gbase + pC.get(sh);
                    }
                    if (PIPE && S >= 16 && !in_lds) {
                        // source in HBM/L2 (channel LLRs or a scratch layer): software-pipelined,
                        // 8 elements (16 loads, 8 KiB per wave) in flight ahead of the compute
                        constexpr int U = 8;
                        double a0[U], b0[U], a1[U], b1[U];
                        auto load = [&](int j, double (&a)[U], double (&b)[U]) {
                            if (in_is_ch) {
#pragma unroll
                                for (int k = 0; k < U; ++k) {
                                    // position j <-> reference beta = bitrev_n(j); (j, j+N/2) <-> (2b', 2b'+1)
                                    unsigned idx = __brev((unsigned)(j + k)) >> (32 - n);
                                    a[k] = CH(in0, idx);
                                    b[k] = CH(in0, idx + 1);
                                }
                            } else {
#pragma unroll
                                for (int k = 0; k < U; ++k) {
                                    a[k] = inp[(size_t)(j + k) * istride];
                                    b[k] = inp[(size_t)(j + k + S) * istride];
                                }
                            }
                        };
                        auto comp = [&](int j, double (&a)[U], double (&b)[U]) {
                            double r[U];
                            if (odd) {
                                if (S > 32 && (j & 31) == 0) cbits = cwp[(size_t)(j >> 5) * 64];
#pragma unroll
                                for (int k = 0; k < U; ++k) r[k] = GN(a[k], b[k], cbits, (j + k) & 31);
                            } else {
#pragma unroll
                                for (int k = 0; k < U; ++k) r[k] = FN(a[k], b[k]);
                            }
#pragma unroll
                            for (int k = 0; k < U; ++k) outp[(size_t)(j + k) * 64] = r[k];
                        };
                        load(0, a0, b0);
                        for (int j = 0; j < S; j += 2 * U) {
                            load(j + U, a1, b1);
                            comp(j, a0, b0);
                            if (j + 2 * U < S) load(j + 2 * U, a0, b0);
                            comp(j + U, a1, b1);
                        }
                    } else if (S >= 4) {
                        for (int j = 0; j < S; j += 4) {
                            double a[4], b[4], r[4];
                            if (in_is_ch) {
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    unsigned idx = __brev((unsigned)(j + k)) >> (32 - n);
                                    a[k] = CH(in0, idx);
                                    b[k] = CH(in0, idx + 1);
                                }
                            } else {
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    a[k] = inp[(size_t)(j + k) * istride];
                                    b[k] = inp[(size_t)(j + k + S) * istride];
                                }
                            }
                            if (odd) {
                                if (S > 32 && (j & 31) == 0) cbits = cwp[(size_t)(j >> 5) * 64];
#pragma unroll
                                for (int k = 0; k < 4; ++k) r[k] = GN(a[k], b[k], cbits, (j + k) & 31);
                            } else {
#pragma unroll
                                for (int k = 0; k < 4; ++k) r[k] = FN(a[k], b[k]);
                            }
#pragma unroll
                            for (int k = 0; k < 4; ++k) outp[(size_t)(j + k) * 64] = r[k];
                        }
                    } else {
                        for (int j = 0; j < S; ++j) {
                            double a, b;
                            if (in_is_ch) {
                                unsigned idx = __brev((unsigned)j) >> (32 - n);
                                a = CH(in0, idx);
                                b = CH(in0, idx + 1);
                            } else {
                                a = inp[(size_t)j * istride];
                                b = inp[(size_t)(j + S) * istride];
                            }
                            double r = odd ? GN(a, b, cbits, j) : FN(a, b);
                            outp[(size_t)j * 64] = r;
                            leaf = r;
                        }
                    }
                    };
                    if (out_lds) generic_body(lds_llr + (size_t)(S - 1) * 64 + lane);
                    else generic_body(g_llr + (size_t)(S - 2 * SL) * 64 + lane);
                    pL.set(sh, lig);
                }
                wave_mem_fence();
                PROF(S > SL ? (odd ? 1 : 2) : (S >= 4 ? 3 : 4))
            }


