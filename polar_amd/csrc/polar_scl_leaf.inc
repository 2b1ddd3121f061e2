// polar_scl_leaf.inc — BODY FRAGMENT of scl_decode_llr_kernel (polar_kernels.hip), included inside its leaf loop after the layer
// visits: rate-0 blocks, continuePaths_FrozenBit / continuePaths_UnfrozenBit (PolarCode.cpp:475-607: fork metrics, ranking,
// kill / clone on the LDS byte stack, history words) and the partial-sum update of the leaf (recursivelyUpdateC, :457-473).
            if (zb) {
                // ---- rate-0 block: Z = 2^zb consecutive frozen leaves whose subtree hangs off the layer of
                // size Z that was just computed. Every decision inside is the frozen 0, so the Z leaf LLRs
                // are a fixed f/g dataflow of that layer (g with u = 0): evaluated level by level in
                // registers (ILP Z/2) instead of Z sequential leaf steps; the path metric is then updated
                // leaf by leaf in order (PolarCode.cpp:475-487), and the block's partial sums (Z zeros) are
                // handed to the layer of size Z exactly as the last leaf's recursivelyUpdateC would.
                const int Z = 1 << zb;
                LANE_CTX
                // one 4-leaf sub-block: values v0..v3 of a size-4 node -> leaves (f,f) (f,g) (g,f) (g,g), then
                // the metric update of those four leaves in order
                auto block4 = [&](double v0, double v1, double v2, double v3) {
                    double lf[4] = {0, 0, 0, 0};
                    if (active) {
                        double a0, a1;
                        FN2(v0, v2, v1, v3, a0, a1);
                        const double b0 = GN(v0, v2, 0u, 0), b1 = GN(v1, v3, 0u, 0);
                        FN2(a0, a1, b0, b1, lf[0], lf[2]);
                        lf[1] = GN(a0, a1, 0u, 0); lf[3] = GN(b0, b1, 0u, 0);
                    }
                    if constexpr (LAT && ED) {
                        // (one codeword per wave: the eight table look-ups of the four leaves in one block — see leaf_terms_ed_block)
                        bool ng[4]; double alz[4], sneg[4], spos[4];
                        leaf_terms_ed_block<4>(lf, actw, tb, ng, alz, sneg, spos);
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (active) pm += ng[i] ? spos[i] : sneg[i];
                    } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        bool ng; double alz, sneg, spos;
                        leaf_terms<ED>(lf[i], active, actw, tb, ng, alz, sneg, spos);
                        if (active) pm += ng ? spos : sneg;
                    }
                    }
                };
                // (one instantiation per address space of the source: a maybe-LDS-maybe-global pointer would
                // turn the loads into FLAT instructions that wait for every outstanding memory operation)
                auto rate0 = [&](const double *yp, auto STR_) {
                    constexpr int YS = decltype(STR_)::value;         // distance between the elements of the layer (LAT: GS)
                    if (zb == 3) {
                        double a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
                        if (active) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const double lo = yp[(size_t)j * YS], hi = yp[(size_t)(j + 4) * YS];
                                a[j] = FN(lo, hi);
                                b[j] = GN(lo, hi, 0u, 0);
                            }
                        }
                        block4(a[0], a[1], a[2], a[3]);
                        block4(b[0], b[1], b[2], b[3]);
                    } else {
                        double y[4] = {0, 0, 0, 0};
                        if (active) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) y[j] = yp[(size_t)j * YS];
                        }
                        block4(y[0], y[1], y[2], y[3]);
                    }
                };
                if constexpr (LAT) rate0(lat_a + (size_t)(Z - 1) * GS + lig, std::integral_constant<int, GS>{});
                else if (Z <= SL) rate0(lds_llr + (size_t)(Z - 1) * 64 + lane, std::integral_constant<int, 64>{});
                else rate0(g_llr + (size_t)(Z - 2 * SL) * 64 + lane, std::integral_constant<int, 64>{});
                const int nu = phi >> zb;                     // node index of the block at its layer
                if ((nu & 1) == 0) {
                    if (active) clsmall &= ~((((u64)1 << Z) - 1ull) << Z);   // column 0 of that layer := 0
                } else {
                    update_c(Z, 0u, nu);
                }
                wave_mem_fence();
                PROF(5)
                phi += Z - 1;
                continue;
            }
            // ---------------- leaf: frozen / unfrozen ----------------
            LANE_CTX
            const u64 below = (1ull << lig) - 1ull;
            const bool frozen = (ctl & 1u) != 0;      // wave-uniform
            unsigned ubit = 0;
            if (frozen) {
                // continuePaths_FrozenBit: PolarCode.cpp:475-487
                // PM += log(1+e^-llr): exactly 0 for llr >= 37, exactly |llr| (+0) for llr <= -37
                bool ng; double alz, sneg, spos;
                if constexpr (LAT && ED) {
                    const double lf1[1] = {leaf}; bool ng1[1]; double al1[1], sn1[1], sp1[1];
                    leaf_terms_ed_block<1>(lf1, actw, tb, ng1, al1, sn1, sp1);
                    ng = ng1[0]; alz = al1[0]; sneg = sn1[0]; spos = sp1[0];
                } else leaf_terms<ED>(leaf, active, actw, tb, ng, alz, sneg, spos);
                if (active) pm += ng ? spos : sneg;
            } else {
                // continuePaths_UnfrozenBit: PolarCode.cpp:489-607
                // (LAT: every lane group holds the same paths — the first group's bits, on the scalar unit)
                const u64 actm = LAT ? (actw & gmask) : ((actw >> gbase) & gmask);
                const int nact = __popcll(actm);
                const int rho = (2 * nact < L) ? 2 * nact : L;
                // ---- fast path (exact): list full and every "good" fork (the bit the leaf LLR favours)
                // beats every "bad" fork of every path => the L survivors are the L good forks, nobody
                // is killed or cloned.  good metric = PM + log(1+e^-|llr|) (the same sum the general
                // path computes); bad metric = PM + log(1+e^|llr|) >= (PM + |llr|)(1 - 2^-40).
                bool lneg; double al;                      // llr < 0, |llr|
                double gm = -__builtin_inf(), bl = __builtin_inf();
                double sneg, spos;                         // log(1+e^-|llr|), log(1+e^|llr|)
                // (a logarithm-free lower bound of |llr| for this test — exponent and mantissa of E — was measured:
                // -1.5 %, the bound is short by up to 0.06 and sends more steps down the ranking path)
                if constexpr (LAT && ED) {
                    const double lf1[1] = {leaf}; bool ng1[1]; double al1[1], sn1[1], sp1[1];
                    leaf_terms_ed_block<1>(lf1, actw, tb, ng1, al1, sn1, sp1);
                    lneg = ng1[0]; al = al1[0]; sneg = sn1[0]; spos = sp1[0];
                } else leaf_terms<ED>(leaf, active, actw, tb, lneg, al, sneg, spos);
                if constexpr (ED) {
                    // a leaf the host marked as weak (control word bit 8: no construction for an ordinary channel leaves it
                    // unfrozen) that comes out below 1e-8: the reference decides on the rounding noise of its own arithmetic
                    // there, which the LLR-domain kernel follows much further down than this one -> fallback pass
                    if (POLAR_UNLIKELY2(ctl & 0x100u)) guard |= __ballot(active && fabs(leaf) > 0.99999999 && fabs(leaf) <= 1.0);
                }
                if (active) {
                    gm = pm + sneg;
                    bl = (pm + al) * 0.99999999999909050530;
                }
                // cheap sufficient test first: the metrics are non-negative doubles, so their HIGH words
                // order like unsigned integers; max / min of those over the group cost one DPP-fused integer
                // instruction per stage and no LDS traffic. Distinct high words decide gmax < bmin for
                // certain; only when they collide (|gmax - bmin| < 2^-20 relative) or the test fails are the
                // exact fp64 reductions run.
                bool fast;
                {
                    unsigned gh = active ? (unsigned)__double2hiint(gm) : 0u;
                    unsigned bh = active ? (unsigned)__double2hiint(bl) : 0xFFFFFFFFu;
                    group_max_min_u32<GS>(gh, bh);
                    if constexpr (LAT) {
                        fast = (nact == 0) || (nact == L && ((__builtin_amdgcn_uicmp(gh, bh, 36) | ~group_result_rows<GS>()) == ~0ull));   // (nact is wave-uniform)
                    } else {
                    const u64 m_ok = __builtin_amdgcn_sicmp(nact, 0, 32) | (__builtin_amdgcn_sicmp(nact, L, 32) & __builtin_amdgcn_uicmp(gh, bh, 36));   // EQ, EQ, ULT
                    fast = ((m_ok | ~group_result_rows<GS>()) == ~0ull);
                    }
                }
                double gmax = 0.0;
                if (!fast) {
                    gmax = group_reduce<GS, true>(gm, lane);
                    const double bmin = group_reduce<GS, false>(bl, lane);
                    fast = wave_all((nact == 0) || (nact == L && gmax < bmin));
                }
                PROF_CNT(8, 1)
                PROF_R1_LEAF(ctl, fast, ((__builtin_amdgcn_sicmp(nact, 0, 32) | __builtin_amdgcn_sicmp(nact, L, 32)) == ~0ull))
                PROF(16)
                if (fast) {      // (marking this likely — the ranking path out of line — measured -0.5 %)
                    PROF_CNT(9, 1)
#ifdef POLAR_MARGIN
                    {
                        const double gx = group_reduce<GS, true>(active ? gm : -__builtin_inf(), lane);
                        const double bx = group_reduce<GS, false>(active ? pm + spos : __builtin_inf(), lane);
                        if (nact == L) mingap = __builtin_fmin(mingap, bx - gx);
                    }
#endif
                    if (active) {
                        ubit = lneg ? 1u : 0u;
                        pm = gm;
                        hword |= ubit << (t & 31);
                    }
                    PROF(17)
                } else {
                double pf0 = __builtin_nan(""), pf1 = __builtin_nan("");
                if (active) {
                    pf0 = -(pm + (lneg ? spos : sneg));     // -(PM + log(1+e^-llr)), PolarCode.cpp:505
                    pf1 = -(pm + (lneg ? sneg : spos));     // -(PM + log(1+e^llr)),  PolarCode.cpp:506
                }
                bool c0 = active, c1 = active;
                const bool need = (2 * nact > L);          // otherwise every fork continues
                const bool full = (nact == L);
                if (POLAR_LIKELY2(!wave_any(need && !full))) {
                    // List full (the usual case). Rank = number of better forks in the reference's order
                    // (metric desc = PM asc, fork index asc on ties, PolarCode.cpp:528-553). A bad fork
                    // whose lower bound is worse than every good fork (bl > gmax) can neither survive nor
                    // outrank a survivor, so only the L good forks and the few "competitive" bad forks
                    // are compared against: 32 LDS broadcasts + a short scalar loop instead of 64.
                    const bool goodbit = lneg;                       // bit the leaf LLR favours
                    const double mg = goodbit ? -pf1 : -pf0;                // PM of my good / bad fork
                    const double mb = goodbit ? -pf0 : -pf1;
                    const bool cbad = active && full && !(bl > gmax);
                    const u64 cbm = __ballot(cbad);
                    bool sg, sbd;
                    if constexpr (GS == 32) {
                        // Two groups of 32 lanes. (1) Every competitive bad fork is ranked on the SCALAR unit: its metric
                        // is read into SGPRs, four wave-wide compares give the masks of the good / competitive bad forks
                        // ordered before it (metric, then fork index 2*path + bit), a population count gives its rank.
                        // (2) The list stays at L, so k surviving bad forks displace the k WORST good forks of the
                        // group; those are peeled off by a DPP maximum over the metrics' high words (non-negative
                        // doubles order like their bit patterns), all lanes sharing the maximal high word at once
                        // when k allows, otherwise the low words and lane numbers decide, on the scalar unit.
                        const u64 actm64 = actw;
                        const u64 gbm = __ballot(goodbit);
                        u64 surv = 0;
                        PROF_CNT(10, 1)
                        PROF_CNT(11, __popcll(cbm))
                        for (u64 mi = cbm; mi; mi &= mi - 1) {
                            const int l_ = __builtin_ctzll(mi);
                            const double s_mb = readlane_d(mb, l_);
                            const u64 grp = 0xFFFFFFFFull << (l_ & 32);
                            const u64 blw = ((1ull << l_) - 1ull) & grp;              // paths below l_ in its group
                            const u64 self_first = ~gbm & (1ull << l_);              // own good fork is bit 0: lower index
                            const u64 lt_g = __builtin_amdgcn_fcmp(mg, s_mb, 4), eq_g = __builtin_amdgcn_fcmp(mg, s_mb, 1);
                            const u64 lt_b = __builtin_amdgcn_fcmp(mb, s_mb, 4), eq_b = __builtin_amdgcn_fcmp(mb, s_mb, 1);
                            const int r = __popcll((lt_g | (eq_g & (blw | self_first))) & grp & actm64) +
                                          __popcll((lt_b | (eq_b & blw)) & grp & cbm);
                            if (r < L) surv |= 1ull << l_;
                        }
                        PROF(18)
                        int k0 = __popcll(surv & 0xFFFFFFFFull), k1 = __popcll(surv >> 32);
                        u64 alive = actm64;
                        const unsigned khi = (unsigned)__double2hiint(mg) + 1u, klo = (unsigned)__double2loint(mg);
                        auto peel = [&](u64 e, int &k) {
                            const int ne = __popcll(e);
                            if (ne == 0) { k = 0; return; }
                            if (ne <= k) { alive &= ~e; k -= ne; return; }
                            for (; k > 0; --k) {                                       // equal high words: low word, then lane
                                int best = -1; unsigned blo = 0;
                                for (u64 q = e; q; q &= q - 1) {
                                    const int l_ = __builtin_ctzll(q);
                                    const unsigned lo_ = (unsigned)__builtin_amdgcn_readlane((int)klo, l_);
                                    if (best < 0 || lo_ >= blo) { best = l_; blo = lo_; }
                                }
                                e &= ~(1ull << best);
                                alive &= ~(1ull << best);
                            }
                        };
                        while (k0 | k1) {
                            const unsigned h0 = __builtin_amdgcn_inverse_ballot_w64(alive) ? khi : 0u;
                            unsigned h = h0;
                            group_max_u32<GS>(h);
                            const unsigned m0 = (unsigned)__builtin_amdgcn_readlane((int)h, 31), m1 = (unsigned)__builtin_amdgcn_readlane((int)h, 63);
                            const u64 eq = __ballot(h0 == (lane < 32 ? m0 : m1)) & alive;
                            if (k0) peel(eq & 0xFFFFFFFFull, k0);
                            if (k1) peel(eq & 0xFFFFFFFF00000000ull, k1);
                        }
                        sg = __builtin_amdgcn_inverse_ballot_w64(alive);
                        sbd = __builtin_amdgcn_inverse_ballot_w64(surv);
                        PROF_CNT(13, (__popcll(surv & 0xFFFFFFFFull) > __popcll(surv >> 32)) ? __popcll(surv & 0xFFFFFFFFull) : __popcll(surv >> 32))
                        PROF(19)
                    } else {
                        sortbuf[lane] = mg;
                        wave_mem_fence();
                        int rg = 0, rb = 0;
                        const double *sb = sortbuf + gbase;
                        // good fork of path i (index 2i + bit) vs my forks (indices 2*lig + ...): it precedes them
                        // on a tie exactly when i < lig (for i == lig see below), so the tie-break folds into the
                        // choice between "<=" and "<"; comparisons produce wave masks, combined on the scalar unit
#pragma unroll 8
                        for (int i = 0; i < GS; ++i) {
                            const double v = sb[i];
                            const u64 below_me = __ballot(lig > i);                    // lanes for which i < lig
                            const u64 lt_g = __builtin_amdgcn_fcmp(v, mg, 4), le_g = __builtin_amdgcn_fcmp(v, mg, 5);
                            const u64 lt_b = __builtin_amdgcn_fcmp(v, mb, 4), le_b = __builtin_amdgcn_fcmp(v, mb, 5);
                            rg += (int)__builtin_amdgcn_inverse_ballot_w64((le_g & below_me) | (lt_g & ~below_me));
                            rb += (int)__builtin_amdgcn_inverse_ballot_w64((le_b & below_me) | (lt_b & ~below_me));
                        }
                        // i == lig: my own good fork is never counted against itself (v < mg is false); against my
                        // bad fork the strict part (mg < mb) was counted above, a tie goes to the lower fork index
                        rb += (mg == mb && !goodbit) ? 1 : 0;
                        PROF(18)
                        // competitive bad forks (few at low SNR, up to all L when garbage paths fill the list):
                        // same scheme from the second half of the exchange buffer, iterations without a
                        // competitive bad fork in any group are skipped on the scalar unit
                        sortbuf[64 + lane] = mb;
                        wave_mem_fence();
                        const double *sbb = sortbuf + 64 + gbase;
                        u64 any_i = 0;                                       // bit i: some group has a competitive bad fork i
#pragma unroll
                        for (int g = 0; g < 64 / GS; ++g) any_i |= (cbm >> (g * GS)) & gmask;
                        PROF_CNT(10, 1)
                        PROF_CNT(11, __popcll(any_i))
#ifdef POLAR_PROFILE
                        {   // statistics only: good forks that some bad fork of their group could displace
                            const double bmin_true = group_reduce<GS, false>(active ? mb : __builtin_inf(), lane);
                            const u64 cgm = __ballot(active && !(mg < bmin_true));
                            u64 any_g = 0;
                            for (int g = 0; g < 64 / GS; ++g) any_g |= (cgm >> (g * GS)) & gmask;
                            PROF_CNT(12, __popcll(any_g))
                        }
#endif
                        for (u64 mi = any_i; mi; mi &= mi - 1) {
                            const int i = __builtin_ctzll(mi);
                            const double v = sbb[i];
                            const u64 mine = __ballot(((cbm >> gbase) >> i) & 1ull);      // lanes whose group's bad fork i competes
                            const u64 below_me = __ballot(lig > i);
                            const u64 lt_g = __builtin_amdgcn_fcmp(v, mg, 4), le_g = __builtin_amdgcn_fcmp(v, mg, 5);
                            const u64 lt_b = __builtin_amdgcn_fcmp(v, mb, 4), le_b = __builtin_amdgcn_fcmp(v, mb, 5);
                            rg += (int)__builtin_amdgcn_inverse_ballot_w64(((le_g & below_me) | (lt_g & ~below_me)) & mine);
                            rb += (int)__builtin_amdgcn_inverse_ballot_w64(((le_b & below_me) | (lt_b & ~below_me)) & mine);
                        }
                        // i == lig: my own bad fork against my good fork: mb < mg cannot hold, a tie goes to the
                        // lower fork index (the bad fork has the lower index when the good bit is 1)
                        rg += (cbad && mg == mb && goodbit) ? 1 : 0;
                        PROF(19)
#ifdef POLAR_PROFILE
                        {   // statistics only: surviving bad forks (= killed good forks) per group, max over the groups
                            const u64 sbm = __ballot(cbad && rb < L);
                            int kmax = 0, ktot = 0;
                            for (int g = 0; g < 64 / GS; ++g) { const int k_ = __popcll((sbm >> (g * GS)) & gmask); kmax = k_ > kmax ? k_ : kmax; ktot += k_; }
                            PROF_CNT(13, kmax)
                            PROF_CNT(14, kmax <= 4 ? 1 : 0)
                            PROF_CNT(15, kmax == 0 ? 1 : 0)
                        }
#endif
                        sg = active && (rg < L);
                        sbd = cbad && (rb < L);
                    }
                    if (full) {
                        c0 = goodbit ? sbd : sg;
                        c1 = goodbit ? sg : sbd;
                    }
#ifdef POLAR_MARGIN
                    {
                        const double ninf = -__builtin_inf(), pinf = __builtin_inf();
                        const double sv = __builtin_fmax(sg ? mg : ninf, sbd ? mb : ninf);
                        const double kv = __builtin_fmin((active && !sg) ? mg : pinf, (active && !sbd) ? mb : pinf);
                        const double sx = group_reduce<GS, true>(sv, lane), kx = group_reduce<GS, false>(kv, lane);
                        if (full) mingap = __builtin_fmin(mingap, kx - sx);
                    }
#endif
                    wave_mem_fence();
                } else {
                    sortbuf[2 * lane] = pf0;
                    sortbuf[2 * lane + 1] = pf1;
                    wave_mem_fence();
                    int r0 = 0, r1 = 0;
                    const double *sb = sortbuf + 2 * gbase;
                    const int i0 = 2 * lig;
                    // stable rank: value descending, fork index 2l+b ascending on ties
                    // (PolarCode.cpp:528-553: "> threshold" first, then "== threshold" in index order)
#pragma unroll 4
                    for (int i = 0; i < 2 * GS; ++i) {
                        const double v = sb[i];
                        r0 += (i < i0) ? (v >= pf0) : (v > pf0);
                        r1 += (i <= i0) ? (v >= pf1) : (v > pf1);
                    }
                    if (need) {
                        c0 = active && (r0 < rho);
                        c1 = active && (r1 < rho);
                    }
                    wave_mem_fence();
                }
                // kills (ascending l) push, then clones (ascending l) pop: PolarCode.cpp:555-570
                const bool kill = active && !c0 && !c1;
                const bool both = c0 && c1;
                const u64 km = (__ballot(kill) >> gbase) & gmask;
                const u64 bm = (__ballot(both) >> gbase) & gmask;
                srcof[lane] = (unsigned char)lig;
                if (POLAR_LIKELY2(wave_all(!active || full))) {
                    // list full before the step => #kills == #clones: the kills are pushed (ascending l) and
                    // popped right back (LIFO) by the clones in ascending l, i.e. the r-th cloner revives the
                    // r-th LARGEST killed index; stack pointer and the entries below are untouched. One LDS
                    // round trip: cloners post their index by rank, killed lanes pick theirs up.
                    if (both) stackv[gbase + __popcll(bm & below)] = (unsigned char)lig;           // rank r -> cloner
                    wave_mem_fence();
                    if (kill) srcof[lane] = stackv[gbase + __popcll(km >> 1 >> lig)];             // #killed above me = my rank from the top
                    wave_mem_fence();
                } else {
                    if (kill) stackv[gbase + sp + __popcll(km & below)] = (unsigned char)lig;
                    sp += __popcll(km);
                    wave_mem_fence();
                    if (both) {
                        int lp = stackv[gbase + sp - 1 - __popcll(bm & below)];
                        srcof[gbase + lp] = (unsigned char)lig;
                    }
                    sp -= __popcll(bm);
                    wave_mem_fence();
                }
                const int src = srcof[lane];
                const bool is_clone = (src != lig);
                PROF(20)
                // PM of the surviving forks: PM + log(1+exp(-+llr)) is the very sum whose negation
                // was ranked (PolarCode.cpp:580-582, 593, 601)
                double pm_new = c0 ? -pf0 : -pf1;
                ubit = c0 ? 0u : 1u;
                if (wave_any(is_clone)) {
                    const int sl = gbase + src;
                    double pm1 = shfl_d(-pf1, sl);
                    u64 a0 = shfl_u64(pL.lo, sl), a1 = shfl_u64(pL.hi, sl);
                    u64 b0 = shfl_u64(pC.lo, sl), b1 = shfl_u64(pC.hi, sl);
                    u64 cs = shfl_u64(clsmall, sl);
                    uint32_t hw = __shfl(hword, sl, 64);
                    int og = __shfl(origin, sl, 64);
                    if (is_clone) {
                        pm_new = pm1; ubit = 1u;
                        pL.lo = a0; pL.hi = a1; pC.lo = b0; pC.hi = b1;
                        clsmall = cs; hword = hw; origin = og;
                    }
                    if constexpr (LAT) {
                        // (the register-resident bottom of the tree: what the leaves of this pair / quad still to come will read)
                        if ((n >= 3) ? ((phi & 1) == 0) : lat_yv) {
                            const double y0_ = shfl_d(lat_y0, sl), y1_ = shfl_d(lat_y1, sl);
                            if (is_clone) { lat_y0 = y0_; lat_y1 = y1_; }
                        }
                        if (n >= 3 && (phi & 3) < 2) {
                            double x_[4];
#pragma unroll
                            for (int k = 0; k < 4; ++k) x_[k] = shfl_d(lat_x[k], sl);
                            if (is_clone) {
#pragma unroll
                                for (int k = 0; k < 4; ++k) lat_x[k] = x_[k];
                            }
                        }
                    }
                }
                active = (active && !kill) || is_clone;
                actw = __ballot(active);
                if (active) {
                    pm = pm_new;
                    hword |= ubit << (t & 31);
                } else {
                    pm = 0.0;   // killPath zeroes the metric (PolarCode.cpp:293-294)
                }
                PROF(21)
                }   // general path
#if POLAR_R1
                if constexpr (ED && !LAT && GS == 32) {
                bool r1_go = false;
                if ((ctl & 0x600u) && !prof_r1_off) {
                    r1_go = fast;
#if POLAR_R1_RANK
                    // (after a ranking step: the list was full in every group that has paths, so it still is)
                    if (!fast && !prof_rank_off) r1_go = ((__builtin_amdgcn_sicmp(nact, 0, 32) | __builtin_amdgcn_sicmp(nact, L, 32)) == ~0ull);   // EQ, EQ
#endif
                }
                if (r1_go) {
                    // ---- rate-1 quad continuation. This leaf is the first of an aligned block of four unfrozen leaves (host mark: no
                    // weak leaf, no history flush before the block's last leaf), the list is full, and the f-chain that came down to this
                    // leaf wrote the layers of size 4 and 2 into every lane's own slots. The leaf step above is complete: by the fast
                    // path (nobody killed or cloned, every path took the bit its leaf favours) or (POLAR_R1_RANK) by a ranking step,
                    // after which a clone holds its source's slot pointers and a path may carry the bit its leaf does not favour. If
                    // the three leaves that follow take the fast path, every path just takes the bit its leaf favours, and the four steps are
                    // one: the leaf values of positions 1..3 are computed here from those two layers, the fast-path test is run
                    // for each of them in order on temporaries, and only if all three pass (in both lane groups) is anything committed.
                    // Otherwise nothing was written — the guard distance of the f-node included, which is kept in a temporary — and the
                    // loop goes on at phi + 1 as ever.
                    //
                    // The layers are read through the slot pointers, as the g-visit of the LDS layers reads them (polar_scl_visits.inc),
                    // and the g-nodes get the bits the walk's partial sums would hold: u0 = the bit this path took at leaf 0 for
                    // g(y0, y1); then (u0 ^ u1, u1) for the two g-nodes of the layer of 4 and u2 for the last leaf, where u1 and u2 are
                    // the sign bits of the leaf values 1 and 2: a leaf on the fast path decides neg = signbit(v) && |v| != 1, and a block
                    // in which a later leaf value of any active lane has |v| == 1.0 (LLR 0: it decides 0 whatever its sign) is left to
                    // the loop. Same g_node_e, same operands, same bits as the walk: the values are the walk's. After a fast leaf 0 the
                    // block is also given up over |leaf 0| == 1.0, as it was when those bits were taken from the operands' signs.
                    PROF_CNT(29, 1)
                    if (!fast) { PROF_CNT(36, 1) R1_CNT(2) }
                    // (the control word of the leaf behind the quad, should it be finished here: asked for now, needed at the commit —
                    // loaded at the top of the step it would be one more scalar held across the layer visits)
                    const uint32_t ctl_r1 = ctlp[phi + 4 < N ? phi + 4 : 0];
                    double lf[3] = {0.0, 0.0, 0.0};
                    double gq = gacc;
                    if (active) {
                        const double *yq = lds_llr + (size_t)1 * 64 + gbase + pL.get(1), *xq = lds_llr + (size_t)3 * 64 + gbase + pL.get(2);      // layers of size 2, 4
                        const double y0 = yq[0], y1 = yq[64], x0 = xq[0], x1 = xq[64], x2 = xq[128], x3 = xq[192];
                        const unsigned s0 = ubit << 31;
                        lf[0] = g_node_e(y0, y1, s0, tb);
                        const unsigned s1 = (unsigned)__double2hiint(lf[0]);
                        const double z0 = g_node_e(x0, x2, s0 ^ s1, tb), z1 = g_node_e(x1, x3, s1, tb);
                        lf[1] = f_node_e_acc(z0, z1, gq);
                        lf[2] = g_node_e(z0, z1, (unsigned)__double2hiint(lf[1]), tb);
                    }
                    // the fast-path tests in leaf order, on temporaries: metric of the good forks so far (pmq), the sufficient
                    // test on the high words alone (see the step above). Where high words collide or the test fails the block is
                    // left to the loop, which runs the exact reductions itself: giving up is always exact.
                    double pmq = pm;
                    auto tests = [&](const auto &lv, u64 m_one, uint32_t &uq) -> bool {
                        constexpr int CNT = (int)(sizeof(lv) / sizeof(double));
                        u64 m_lt = ~0ull;
                        uq = 0;
#pragma unroll
                        for (int i_ = 0; i_ < CNT; ++i_) {
                            bool ng1; double al1, sn1, sp1;
                            leaf_terms<ED>(lv[i_], active, actw, tb, ng1, al1, sn1, sp1);
                            const double gq_ = pmq + sn1, bq_ = (pmq + al1) * 0.99999999999909050530;
                            unsigned gh_ = active ? (unsigned)__double2hiint(gq_) : 0u, bh_ = active ? (unsigned)__double2hiint(bq_) : 0xFFFFFFFFu;
                            group_max_min_u32<GS>(gh_, bh_);
                            m_lt &= __builtin_amdgcn_uicmp(gh_, bh_, 36);                          // ULT
                            m_one |= __builtin_amdgcn_fcmp(fabs(lv[i_]), 1.0, 1);                  // OEQ
                            pmq = gq_;
                            uq |= (ng1 ? 1u : 0u) << i_;
                        }
                        const u64 m_okq = __builtin_amdgcn_sicmp(nact, 0, 32) | (__builtin_amdgcn_sicmp(nact, L, 32) & m_lt);
                        return ((m_okq | ~group_result_rows<GS>()) == ~0ull) && (m_one & actw) == 0;
                    };
                    uint32_t uq;
                    const bool pass = tests(lf, fast ? __builtin_amdgcn_fcmp(fabs(leaf), 1.0, 1) : 0ull, uq);
                    if (pass) {
                        PROF_CNT(30, 1)
                        PROF_CNT(8, 3)
                        PROF_CNT(9, 3)
                        PROF_R1_COMMIT
                        if (fast) { R1_CNT(0) } else { PROF_CNT(37, 1) R1_CNT(3) }
                        const uint32_t u1 = uq & 1u, u2 = (uq >> 1) & 1u, u3 = uq >> 2;
                        if (active) {
                            pm = pmq;
                            hword |= (u1 << ((t + 1) & 31)) | (u2 << ((t + 2) & 31)) | (u3 << ((t + 3) & 31));
                        }
                        gacc = gq;
                        // the quad's partial sums, as the four calls of the leaf's own update would have left them: after leaf 1
                        // the layer of size 2 holds (u0 ^ u1, u1), after leaf 3 the layer of size 4 gets that pair XOR (u2 ^ u3, u3)
                        // followed by (u2 ^ u3, u3); from there exactly as the rate-0 block hands over its zeros
                        uint32_t X = (ubit ^ u1 ^ u2 ^ u3) | ((u1 ^ u3) << 1) | ((u2 ^ u3) << 2) | (u3 << 3);
                        int Sx = 4, adv = 3;
                        uint32_t ctl_after = ctl_r1;
                        bool octet_open = (ctl & 0x600u) == 0x600u;       // (instrumented build: the octet's leaf 4 is still a loop step)
                        (void)octet_open;
#if POLAR_R1_CHAIN
                        if constexpr (LDS_LOG >= 3) {
                        if ((ctl & 0x600u) == 0x600u && !prof_chain_off) {
                            // ---- the second quad of a marked octet in the same step (rb == 3: no history flush before the octet's
                            // last leaf). The quad just finished is the left half of the octet: X is column 0 of the layer of 4, and
                            // the g-visit of that layer at leaf 4 would form its right half from the layer of 8 — read through its
                            // slot pointer — with exactly these bits, the f-chain below it the layer of 2 and leaf 4. Here all of
                            // that stays in registers; leaf 4 gets the same high-word test as the later leaves, leaves 5 .. 7 the
                            // continuation above. If all four pass, eight leaves are committed at once and the octet's partial sums
                            // go to the layer of 8 as a rate-0 block of 8 hands over its zeros: (X ^ X', X') for the two quads'
                            // X, X'. (The layers of size 4 and 2 are not stored: nothing reads them before the next visit of the
                            // layer of 4 rewrites them, as behind a rate-0 block of 8.) If anything fails nothing further is
                            // written: the state after the first quad is a committed one, and the loop goes on at leaf 4.
                            PROF_CNT(38, 1)
                            R1_CNT(4)
                            const uint32_t ctl_r2 = ctlp[phi + 8 < N ? phi + 8 : 0];
                            double lc[4] = {0.0, 0.0, 0.0, 0.0};
                            double gq2 = gq;
                            if (active) {
                                const double *wq = lds_llr + (size_t)7 * 64 + gbase + pL.get(3);      // layer of size 8
                                double wa[4], wb[4], w[4];
#pragma unroll
                                for (int j = 0; j < 4; ++j) { wa[j] = wq[(size_t)j * 64]; wb[j] = wq[(size_t)(j + 4) * 64]; }
#pragma unroll
                                for (int j = 0; j < 4; ++j) w[j] = g_node_e(wa[j], wb[j], X << (31 - j), tb);
                                const double y0 = f_node_e_acc(w[0], w[2], gq2), y1 = f_node_e_acc(w[1], w[3], gq2);
                                lc[0] = f_node_e_acc(y0, y1, gq2);
                                const unsigned s0 = (unsigned)__double2hiint(lc[0]);
                                lc[1] = g_node_e(y0, y1, s0, tb);
                                const unsigned s1 = (unsigned)__double2hiint(lc[1]);
                                const double z0 = g_node_e(w[0], w[2], s0 ^ s1, tb), z1 = g_node_e(w[1], w[3], s1, tb);
                                lc[2] = f_node_e_acc(z0, z1, gq2);
                                lc[3] = g_node_e(z0, z1, (unsigned)__double2hiint(lc[2]), tb);
                            }
                            uint32_t uc;
                            if (tests(lc, 0ull, uc)) {
                                PROF_CNT(39, 1)
                                PROF_CNT(8, 4)
                                PROF_CNT(9, 4)
                                R1_CNT(5)
                                R1_CNT(0)
                                const uint32_t u4 = uc & 1u, u5 = (uc >> 1) & 1u, u6 = (uc >> 2) & 1u, u7 = uc >> 3;
                                if (active) {
                                    pm = pmq;
                                    hword |= (u4 << ((t + 4) & 31)) | (u5 << ((t + 5) & 31)) | (u6 << ((t + 6) & 31)) | (u7 << ((t + 7) & 31));
                                }
                                gacc = gq2;
                                const uint32_t X2 = (u4 ^ u5 ^ u6 ^ u7) | ((u5 ^ u7) << 1) | ((u6 ^ u7) << 2) | (u7 << 3);
                                X = (X ^ X2) | (X2 << 4);
                                Sx = 8; adv = 7;
                                ctl_after = ctl_r2;
                                octet_open = false;
                            }
                        }
                        }
#endif
                        PROF_R1_OCTET(octet_open)
                        const int nu = phi >> (Sx == 8 ? 3 : 2);
                        if ((nu & 1) == 0) {
                            if (active) clsmall = (Sx == 8) ? ((clsmall & ~(0xFFull << 8)) | ((u64)X << 8)) : ((clsmall & ~(0xFull << 4)) | ((u64)X << 4));
                        } else {
                            update_c(Sx, X, nu);
                        }
                        wave_mem_fence();
                        t += adv;
                        phi += adv;
                        ctl_next = ctl_after;
                        r1_done = true;
                    } else {
                        if (fast) { R1_CNT(1) }
                    }
                    PROF(28)
                }
                }
#endif
                // every 32 unfrozen steps the decision word is stored together with the slot (`origin`) that
                // holds this path's previous word: a linked list per path, walked once at the end, so that
                // neither clones nor flushes ever copy history (the reference copies it on every clone,
                // PolarCode.cpp:574)
                if (POLAR_UNLIKELY2((t & 31) == 31)) {
                    const int w = (int)(t >> 5);
                    if (active) {
                        g_hist[(size_t)w * CST + POLAR_CL] = hword;
                        g_horg[(size_t)w * CST + POLAR_CL] = (uint32_t)origin;
                        origin = lig;
                        hword = 0;
                    }
                    wave_mem_fence();
                }
                ++t;
            }

            PROF(frozen ? 5 : 6)
            // ---------------- partial sums ----------------
#if POLAR_R1
            if (r1_done) {
                // (a rate-1 quad finished in one step has handed its partial sums over itself)
            } else
#endif
            if ((phi & 1) == 0) {
                // left leaf: column 0 of C_n (size 1) lives at bit 1 of clsmall
                if (active) clsmall = (clsmall & ~2ull) | ((u64)ubit << 1);
            } else {
                update_c(1, ubit, phi);
            }
            PROF(7)
