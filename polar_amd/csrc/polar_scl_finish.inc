// polar_scl_finish.inc — BODY FRAGMENT of scl_decode_llr_kernel (polar_kernels.hip), included after the leaf loop of a codeword
// group: last history word, crc_check + findMostProbablePath (PolarCode.cpp:93-108, 609-644), the K info bits, guard flags.
        // ---------------- last (partial) history word ----------------
        const int Wused = (int)((t + 31) >> 5);
        if ((t & 31) != 0 && active) {
            g_hist[(size_t)(Wused - 1) * CST + POLAR_CL] = hword;
            g_horg[(size_t)(Wused - 1) * CST + POLAR_CL] = (uint32_t)origin;
        }
        wave_mem_fence();

        // ---------------- findMostProbablePath + crc_check: PolarCode.cpp:609-644, 93-108 ----------------
        // crc_check walks the path's word list backwards: parity of (word & mask_i) per CRC row
        bool pass = true;
        if (p.crc > 0) {
            uint32_t acc = 0;
            if (active) {
                int cur = lig;
                for (int w = Wused - 1; w >= 0; --w) {
                    const uint32_t hw = g_hist[(size_t)w * CST + POLAR_CGB + cur];
                    cur = (int)(g_horg[(size_t)w * CST + POLAR_CGB + cur] & (GS - 1));
                    for (int i = 0; i < p.crc; ++i)
                        acc ^= (uint32_t)(__popc(hw & p.crc_mask[(size_t)i * p.W + w]) & 1) << i;
                }
            }
            pass = (acc == 0);
        }
        const u64 passm = (__ballot(active && pass) >> gbase) & gmask;
        const bool cand = active && (pass || passm == 0);      // :640-643 fall back to "no CRC"
        double key = (cand && pm < 1.7976931348623157e308) ? pm : __builtin_inf();
        int kidx = lig;
#pragma unroll
        for (int off = GS / 2; off >= 1; off >>= 1) {
            double ok = shfl_d(key, lane ^ off);
            int oi = __shfl(kidx, lane ^ off, 64);
            if (ok < key || (ok == key && oi < kidx)) { key = ok; kidx = oi; }
        }
        // no candidate with PM < DBL_MAX: the reference returns l_p = 0 (PolarCode.cpp:611,626)
        const int win = (key < __builtin_inf()) ? kidx : 0;
#ifdef POLAR_MARGIN
        double fingap;
        {   // final selection: runner-up candidate metric - winner's
            const double mine = (cand && pm < 1.7976931348623157e308 && lig != win) ? pm : __builtin_inf();
            fingap = group_reduce<GS, false>(mine, lane) - key;
        }
#endif
        const double pm_win = shfl_d(pm, gbase + win);
        // No candidate with a finite metric (every path met a frozen leaf with llr < -709.78: the reference's log(1+e^-llr)
        // is +inf there) AND the list never filled (more list entries than 2^K paths): the reference's l_p = 0 is a path that
        // was never activated, its info array still holds the zeros of initializeDataStructures (PolarCode.cpp:195-230).
        // (Found by tools/fuzz_parity.py; this read used to return whatever an earlier codeword left in the slot.)
        const bool win_active = __shfl((int)active, gbase + win, 64) != 0;
#ifdef POLAR_LIST_OUT
        {   // ---------------- list output: every surviving path instead of the winner alone (DESIGN.md §8e) ----------------
            static_assert(!ED && !LAT && !PIPE, "the list-output unit instantiates the LLR-domain batch kernel only");
            (void)pm_win;
            // Row of a path = how many lanes of its group come before it: active paths first, then CRC pass before fail, then the
            // smaller metric (+inf last), then the lower lane — the winner selection's own tie-break. A comparison count over the
            // group: GS - 1 shuffles of (metric, class) per lane, no sort network. Inactive lanes take the rows behind the active
            // ones in lane order: the padded rows n_active .. L-1 are theirs.
            const bool ok = active && pass;
            const int cls = active ? (ok ? 0 : 1) : 2;
            const double km = active ? pm : __builtin_inf();
            int rank = 0;
            for (int j = 1; j < GS; ++j) {
                const int oi = (lig + j) & (GS - 1);
                const double om = shfl_d(km, gbase + oi);
                const int oc = __shfl(cls, gbase + oi, 64);
                rank += (oc < cls || (oc == cls && (om < km || (om == km && oi < lig)))) ? 1 : 0;
            }
            const int n_act = __popcll((__ballot(active) >> gbase) & gmask);
            const int win_row = __shfl(rank, gbase + win, 64);
            // every active path walks its OWN word list into its own column of g_tb
            if (active) {
                int cur = lig;
                for (int w = Wused - 1; w >= 0; --w) {
                    g_tb[(size_t)w * CST + POLAR_CL] = g_hist[(size_t)w * CST + POLAR_CGB + cur];
                    cur = (int)(g_horg[(size_t)w * CST + POLAR_CGB + cur] & (GS - 1));
                }
            }
            wave_mem_fence();
            // path by path: the lanes of the group stride over the K bytes of ONE row (consecutive bytes per store instruction), the
            // words come from that path's column
            const size_t row0 = (size_t)(valid ? cw : 0) * (size_t)L;
            for (int j = 0; j < GS; ++j) {
                const int rj = __shfl(rank, gbase + j, 64);
                const bool aj = __shfl((int)active, gbase + j, 64) != 0;
                if (valid && rj < L) {
                    uint8_t *dst = p.list_cand + (row0 + (size_t)rj) * (size_t)K;
                    for (int b = lig; b < K; b += GS) {
                        uint8_t v = 0;
                        if (aj) {
                            const unsigned r = p.info_rank[b];
                            v = (uint8_t)((g_tb[(size_t)(r >> 5) * CST + POLAR_CGB + j] >> (r & 31)) & 1u);
                        }
                        dst[b] = v;
                    }
                }
            }
            if (valid && rank < L) {
                if (p.list_pm) p.list_pm[row0 + (size_t)rank] = km;
                if (p.list_crc) p.list_crc[row0 + (size_t)rank] = ok ? (uint8_t)1 : (uint8_t)0;
            }
            if (valid && lig == 0) {
                if (p.list_nact) p.list_nact[cw] = n_act;
                // (the reference's l_p = 0 when no candidate has a finite metric: a row like any other if that path is active, no row
                // at all — the all-zero word — if the list never filled)
                if (p.list_win) p.list_win[cw] = win_active ? win_row : -1;
            }
            wave_mem_fence();
        }
#elif defined(POLAR_ADAPT_OUT)
        {   // ---------------- one stage of the adaptive decode (DESIGN.md §8g) ----------------
            static_assert(!ED && !LAT && !PIPE, "the adaptive unit instantiates the LLR-domain batch kernel only");
            // accepted: the winner is an active path AND itself passes the CRC (the "no path passes, take the best anyway" winner of
            // :640-643 is not). Group-uniform. A codeword that is neither accepted nor in the last stage writes nothing of its word —
            // no history walk, no K byte stores —, only its retry byte.
            const bool accepted = win_active && __shfl((int)pass, gbase + win, 64) != 0;
            const bool deliver = accepted || p.ad_last != 0;
            if (deliver) {
                int cur = win;
                for (int w = Wused - 1; w >= 0; --w) {
                    g_tb[(size_t)w * CST + POLAR_CL] = g_hist[(size_t)w * CST + POLAR_CGB + cur];
                    cur = (int)(g_horg[(size_t)w * CST + POLAR_CGB + cur] & (GS - 1));
                }
            }
            wave_mem_fence();
            if (valid && deliver) {
                for (int b = lig; b < K; b += GS) {
                    unsigned r = p.info_rank[b];
                    uint32_t wd = g_tb[(size_t)(r >> 5) * CST + POLAR_CL];
                    p.out[(size_t)cw * K + b] = win_active ? (uint8_t)((wd >> (r & 31)) & 1u) : (uint8_t)0;
                }
                if (lig == 0) {
                    // (no winner row — the reference's never-activated path 0 —: no metric either, +inf like the list's padding)
                    if (p.pm_out) p.pm_out[cw] = win_active ? pm_win : __builtin_inf();
                    if (p.ad_stage) p.ad_stage[cw] = (uint8_t)p.ad_s;
                    if (p.ad_crc) p.ad_crc[cw] = accepted ? (uint8_t)1 : (uint8_t)0;
                }
            }
            // every decoded codeword, every stage: a byte left by an earlier stage or call is never read as current
            if (valid && lig == 0) p.ad_retry[cw] = deliver ? (uint8_t)0 : (uint8_t)1;
            wave_mem_fence();
        }
#else
        if (valid) {
#if !defined(POLAR_PROFILE) && !defined(POLAR_SLOTHIST)
            if (p.pm_out && lig == 0) p.pm_out[cw] = pm_win;
#endif
        }
        {   // the winner's words, in order, into this lane's own column of g_tb (every lane of the group walks
            // the same list, so the loads are broadcasts), then the K info bits by unfrozen rank
            int cur = win;
            for (int w = Wused - 1; w >= 0; --w) {
                g_tb[(size_t)w * CST + POLAR_CL] = g_hist[(size_t)w * CST + POLAR_CGB + cur];
                cur = (int)(g_horg[(size_t)w * CST + POLAR_CGB + cur] & (GS - 1));   // (stale slots of idle groups stay in range)
            }
            wave_mem_fence();
        }
        if (valid) {
            for (int b = LAT ? lane : lig; b < K; b += LAT ? 64 : GS) {
                unsigned r = p.info_rank[b];
                uint32_t wd = g_tb[(size_t)(r >> 5) * CST + POLAR_CL];
                p.out[(size_t)cw * K + b] = win_active ? (uint8_t)((wd >> (r & 31)) & 1u) : (uint8_t)0;
            }
        }
        if constexpr (ED) {
            // codewords with an undecidable |x| < 40 test go to the LLR-domain kernel (host: fallback pass)
            guard |= __ballot(gacc <= ED_GACC_FLAG);
            if constexpr (LAT) { if (valid && lane == 0) p.flags[cw] = (guard != 0) ? 1 : 0; }      // (no conversion pass has cleared it)
            else if (valid && lig == 0 && ((guard >> gbase) & gmask) != 0) p.flags[cw] = 1;
        }
        wave_mem_fence();
#endif  // POLAR_LIST_OUT
#ifdef POLAR_MARGIN
        if (valid && lig == 0 && K >= 16) {      // (overwrites the first 16 info bytes: this build measures, it does not decode)
            double *o = reinterpret_cast<double *>(p.out + (size_t)cw * K);
            o[0] = mingap; o[1] = fingap;
        }
        wave_mem_fence();
#endif
