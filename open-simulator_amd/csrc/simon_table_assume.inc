// simon_table_assume.inc -- the assume of the score-table kernel's scheduling cycle: NodeInfo.AddPod (V/framework/types.go:482-508), the table
// column of the touched node and its summary entries.  A fragment of table_kernel's loop body (simon_table.hip includes it where a branch of
// the cycle has chosen its node, see there); it names the loop body's variables and, as the chosen node,
//   scanned, bound, pstar, dstar, res, top, m16q[], e16q[]
// -- variables of the loop body or parameters of the lambda around it.
            TPROF(3);                                                  // winner info
            // Position order is canonical order inside a class only: do entries of ANOTHER class reach the same total?  Then the
            // first maximum in CANONICAL order decides (static per-class node lists, L2-hot).
            auto tie_with_other_class = [&]() -> bool {
                // (no short-circuit: `||` / `&&` over the lanes' entries compiled to an EXEC region and a compare of a materialised flag;
                // plain mask logic ends on the scalar compare of the ballot)
                bool other = false;
#pragma unroll
                for (int q = 0; q < NBQ; ++q) other |= ((kStraight ? e16q[q] : m16q[q] >> UB) == top) & (bcls[q] != dstar);   // duplicates carry entry 0's class
                return __ballot(other) != 0;
            };
            auto canonical_first = [&]() -> int {
#ifdef SIMON_TABLE_PROFILE
                tp_acc[7] += 1;                                        // how often the canonical tie-break runs
#endif
                unsigned key2 = 0;
                int canon[NBQ];
#pragma unroll
                for (int q = 0; q < NBQ; ++q) {
                    const int pq = (q * 64 + lane) * UNIT + (UNIT - 1) - (int)(m16q[q] & UMASK);
                    const bool tied = (m16q[q] >> UB) == top && q * 64 + lane < nun;
                    if constexpr (LDSX) canon[q] = tied ? (int)sx_canon[pq] : (int)PMASK;
                    else {
                    canon[q] = tied ? cls_list[rk_off + (unsigned)((binfo[q] & 0xFFFF) - 8192 + pq)] : (int)PMASK;
                    if (ranked && tied) canon[q] = gp(cold->rk_rank)[(size_t)s * (size_t)cold->N + canon[q]];
                    }
                }
#pragma unroll
                for (int q = 0; q < NBQ; ++q) {
                    const int pq = (q * 64 + lane) * UNIT + (UNIT - 1) - (int)(m16q[q] & UMASK);
                    if ((m16q[q] >> UB) == top && q * 64 + lane < nun) key2 = max(key2, ((PMASK - (unsigned)canon[q]) << KB) | (unsigned)pq);
                }
                key2 = wave_max_u32(key2);
                return (int)(key2 & PMASK);
            };
            // Generations 4 / 5 speculate: the loads of the first maximum in POSITION order go out first and the tie check runs while
            // they are in flight (it fires on 0.2 % of the cycles of config 3).  The REST instantiation resolves the tie BEFORE it
            // loads: its problems split node classes into nodes with / without devices -- twin classes of one shape that tie on
            // every other cycle (config 5: 49 %), and a lost speculation costs a second round trip to the scenario's workspace.
            if (TIE_FIRST && scanned && __builtin_expect(tie_with_other_class(), 0)) {
                const int p2 = canonical_first();
                if (p2 != pstar) {
                    pstar = p2;
                    const int info = winner_info(pstar >> UB);
                    dstar = info >> 16;
                    res = (info & 0xFFFF) - 8192 + pstar;
                }
            }
            NodeState* stp = g_state + pstar;                          // (kept for the store: one 64-bit scalar address per cycle)
            NodeState st = *stp;
            // (round 10, straight-line instantiations: the state's load goes out AHEAD of the row and the byte -- left to the scheduler the 16-byte row went
            // first, and the state update, its store and the whole evaluation waited for the row's six or seven cache lines, which they do not read.
            // Vector loads return in order: with the state first its wait is vmcnt(2), and the row and the byte are waited for at the patch.
            // Not with the workspace in LDS: nothing leaves the chip there, and the barrier alone cost config 3 at 64 scenarios 0.3 %)
            if constexpr (kStraight && !LDSWS) __builtin_amdgcn_sched_barrier(0);
            // A table row is named by its 32-bit byte offset: row and byte accesses are uniform base + lane offset, and the byte's address is one
            // add, shared by the load and the store.  MANY keeps 64-bit pointers: with its eighteen row accesses per cycle the offsets measured
            // slower (config 3 with 200 signatures 83.4 -> 87.7 ms; the others gain, config 3 13.1 -> 12.7 ms).
            using RowRef = std::conditional_t<MANY, unsigned char*, unsigned>;
            auto row_ref = [&](unsigned off) -> RowRef { if constexpr (MANY) return g_tile + off; else return off; };
            auto row_vec = [&](RowRef r) -> uint4 { if constexpr (MANY) return *(const uint4*)r; else return *(const uint4*)(g_tile + r); };
            auto row_byte = [&](RowRef r, int i) -> unsigned char& { if constexpr (MANY) return r[i]; else return g_tile[r + (unsigned)i]; };
            // (round 9, straight-line instantiations: the byte's offset is formed once and serves the load and the store -- left to the compiler, the
            // load took an `or` and the store an `add` of the same two values.  It is made opaque BEHIND the loads: an inline-asm result costs the
            // instructions that read it next a hazard s_nop each, and ahead of the loads those sat on the cycle's chain)
            // (a byte reference: the byte's own offset where it is kept, else the row's -- what refresh_sig is handed either way)
            auto byte_ref = [&](RowRef r, int i) -> RowRef {
                if constexpr (kStraight) return r + (unsigned)i;
                else return r;
            };
            auto byte_at = [&](RowRef b, int i) -> unsigned char& { if constexpr (kStraight) return g_tile[b]; else return row_byte(b, i); };
            RowRef rowp[KQ], bytep[KQ];
            uint4 T[KQ];
            uint2 F[KQ];                                               // COARSE: the four per-16 entries of (signature, touched 64 positions)
            unsigned oldq[KQ];
#pragma unroll
            for (int q = 0; q < KQ; ++q) {
                rowp[q] = row_ref(tile_blk((unsigned)(pstar >> 4)) + koff[q]);
                T[q] = row_vec(rowp[q]);
                bytep[q] = byte_ref(rowp[q], pstar & 15);
                oldq[q] = byte_at(bytep[q], pstar & 15);                         // this signature's byte before the cycle (same cache line as the row)
                if (COARSE) F[q] = *(const uint2*)(g_fine + ((unsigned)(pstar >> 6) * (unsigned)K + (unsigned)kk[q]) * 4u);
            }
            // Fold (TableScalars::static_tables & kStFold): required anti-affinity / host ports on node-level keys.  The landing pod's signature
            // names the signatures that may not use this node any more (TableCold::foldx, one bit per signature): their bytes go to 0 with
            // the refresh below and stay there -- the table's monotone infeasibility; summaries and counters follow as for a full node.
            // Only the two-level instantiations without the REST rows that know pinned pods carry the code (the host picks them for such
            // problems): the kernels of the benchmark configurations stay as they are.
            constexpr bool kFoldable = COARSE && !REST && HAS_PIN;   // (launch_table sends a problem with the fold to the HAS_PIN instantiations)
            const bool fold = kFoldable && (sc.static_tables & kStFold);
            const unsigned KW = ((unsigned)K + 31u) >> 5;
            unsigned xfold[KQ];
            if constexpr (kFoldable) {
                if (__builtin_expect(fold, 0)) {                      // (a uniform branch)
#pragma unroll
                    for (int q = 0; q < KQ; ++q) xfold[q] = gp(cold->foldx)[(unsigned)r_sig * KW + ((unsigned)kk[q] >> 5)];
                }
            }
            // MANY: the rows of the signatures beyond the register-resident ones, same round trip (uniform group conditions)
            unsigned xfg[NG ? NG : 1][KQ];
            RowRef rowg[NG ? NG : 1][KQ];
            uint4 Tg[NG ? NG : 1][KQ];
            uint2 Fg[NG ? NG : 1][KQ];
            unsigned oldg[NG ? NG : 1][KQ];
            int kg[NG ? NG : 1][KQ];
            if constexpr (MANY) {
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    if (128 * (g + 1) < K) {
#pragma unroll
                        for (int q = 0; q < KQ; ++q) {
                            const int k = 128 * (g + 1) + 64 * q + lane;
                            kg[g][q] = k < K ? k : 0;
                            rowg[g][q] = row_ref(tile_blk((unsigned)(pstar >> 4)) + (unsigned)kg[g][q] * KS);
                            Tg[g][q] = row_vec(rowg[g][q]);
                            oldg[g][q] = row_byte(rowg[g][q], pstar & 15);
                            Fg[g][q] = *(const uint2*)(g_fine + ((unsigned)(pstar >> 6) * (unsigned)K + (unsigned)kg[g][q]) * 4u);
                            if (__builtin_expect(fold, 0)) xfg[g][q] = gp(cold->foldx)[(unsigned)r_sig * KW + ((unsigned)kg[g][q] >> 5)];
                        }
                    }
                }
            }
            uint2 z = make_uint2(0, 0);
            if (!NZEQ) z = g_nz[pstar];
            if constexpr (kStraight) {
                // The scan's winner: its class and record index are read off the lanes' entry constants BEHIND the loads of its state, row and
                // byte -- only the position feeds their addresses, and the memory round trip is the longest link of the cycle's chain.
                if (scanned) {
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int q = 0; q < KQ; ++q) asm volatile("" : "+v"(bytep[q]));
                    const int info = winner_info(pstar >> UB);
                    dstar = info >> 16;
                    res = (info & 0xFFFF) - 8192 + pstar;              // index into cls_list
                }
            }
            if (!TIE_FIRST && scanned && __builtin_expect(tie_with_other_class(), 0)) {   // rare: first maximum in CANONICAL order
                const int p2 = canonical_first();
                if (p2 != pstar) {                                     // the speculated winner loses the tie: load the real one
                    pstar = p2;
                    const int info = winner_info(pstar >> UB);
                    dstar = info >> 16;
                    res = (info & 0xFFFF) - 8192 + pstar;
                    stp = g_state + pstar;
                    st = *stp;
                    if constexpr (kStraight && !LDSWS) __builtin_amdgcn_sched_barrier(0);   // (the same order as above: the two paths meet in front of the state's wait)
#pragma unroll
                    for (int q = 0; q < KQ; ++q) {
                        rowp[q] = row_ref(tile_blk((unsigned)(pstar >> 4)) + koff[q]);
                        T[q] = row_vec(rowp[q]);
                        bytep[q] = byte_ref(rowp[q], pstar & 15);
                        oldq[q] = byte_at(bytep[q], pstar & 15);
                        if (COARSE) F[q] = *(const uint2*)(g_fine + ((unsigned)(pstar >> 6) * (unsigned)K + (unsigned)kk[q]) * 4u);
                    }
                    if (!NZEQ) z = g_nz[pstar];
                }
            }
            const int blk = pstar >> 4, pos = pstar & 15;
            int c15 = 15 - pos;                                        // block_key16_patched's constant of the touched position
            if constexpr (kStraight) asm volatile("" : "+s"(c15));  // (uniform: a scalar subtract, not a vector xor per signature)
            RestLoads RL{};
            if (REST && __builtin_expect(rw != 0, 0)) RL = rest_assume_load(pstar, r_nrows, rowv, bound ? -1 : r_gs, r_xs);
            // GPU fold: the landing position's devices travel with the assume's loads (uniform addresses)
            uint4 gfa = make_uint4(0, 0, 0, 0), gfb = make_uint4(0, 0, 0, 0);
            unsigned gft = 0;
            int gfc = 0;
            if constexpr (kGpuFoldable) {
                if (__builtin_expect(gfold, 0)) {
                    gfc = g_fc[pstar]; gft = g_ft[pstar];
                    gfa = *(const uint4*)(g_fu + (size_t)pstar * 8); gfb = *(const uint4*)(g_fu + (size_t)pstar * 8 + 4);
                }
            }
            SpreadLoads SPL{0u, 0u, false};
            if (SPREAD && sp_match != 0) SPL = spread_count_load(pstar, dstar, res, spv, spt, sp_soft, sp_match);
            const ShapeRow sh = shape_of(dstar);
            unsigned snq[KQ];
#pragma unroll
            for (int q = 0; q < KQ; ++q) snq[q] = s_sn[kk[q] * Cn + dstar];
            // byte -> u16 expansion selectors of the touched block row with the new byte already in place (kSel, above)
            const uint4 selA = sel_tab[pos * 2], selB = sel_tab[pos * 2 + 1];
            TPROF_WAIT_LDS; TPROF(4);                                  // loads issued; shape row and class term arrived (LDS)
            if constexpr (kStraight && !LDSWS) { TPROF_WAIT_STATE(KQ * (COARSE ? 3 : 2) + (NZEQ ? 0 : 1)); TPROF(20); }   // node state arrived (the loads issued behind it still in flight)
            TPROF_WAIT_MEM; TPROF(5);                                  // ... and table row and byte arrived (L2 / HBM)
            const int sl = r_sig & 63;
            const bool hiq = KQ > 1 && (r_sig >> 6);
            unsigned add_c, add_m, addz_c = 0, addz_m = 0;
            if (MANY && __builtin_expect(r_sig >= 64 * KQ, 0)) {       // a signature beyond the register-resident ones (K > 128): its row
                const SigRow rs = sigs[r_sig];                         // (uniform index: scalar loads)
                add_c = (unsigned)rs.req_c; add_m = (unsigned)rs.req_m; addz_c = (unsigned)rs.nz_c; addz_m = (unsigned)rs.nz_m;
            } else {
                add_c = (unsigned)(hiq ? __builtin_amdgcn_readlane((int)my_add_c[KQ - 1], sl) : __builtin_amdgcn_readlane((int)my_add_c[0], sl));
                add_m = (unsigned)(hiq ? __builtin_amdgcn_readlane((int)my_add_m[KQ - 1], sl) : __builtin_amdgcn_readlane((int)my_add_m[0], sl));
                if (!NZEQ) {
                    addz_c = (unsigned)(hiq ? __builtin_amdgcn_readlane((int)my_addz_c[KQ - 1], sl) : __builtin_amdgcn_readlane((int)my_addz_c[0], sl));
                    addz_m = (unsigned)(hiq ? __builtin_amdgcn_readlane((int)my_addz_m[KQ - 1], sl) : __builtin_amdgcn_readlane((int)my_addz_m[0], sl));
                }
            }
            st.rq_c += add_c;
            st.rq_m += add_m;
            st.freep -= 1u;
            double nzc = 0.0, nzm = 0.0;
            if (!NZEQ) {
                z.x += addz_c;
                z.y += addz_m;
                if (lane == 0) g_nz[pstar] = z;
                nzc = (double)z.x; nzm = (double)z.y;
            }
            // (kLanesStore: every lane holds the same state and stores it to the same address -- no EXEC region around the store, and the wait for
            // the table byte below no longer waits for this store to be acknowledged, see simon_table.hip)
            // (kFitMask: the free-slot compare of the evaluation's fit, taken here, ahead of the barrier below: left to the scheduler it came last and the
            // slot count lived through the evaluation, one VGPR -- for config 3's fused kernel the one across a waves-per-SIMD step)
            unsigned long long free_m;                                 // (kFitMask only)
            if constexpr (kFitMask) free_m = __ballot((int)st.freep >= 1);
            if (kLanesStore || lane == 0) *stp = st;
            // (the region's end was a boundary for the instruction scheduler as well: without one here it interleaves the state update with the
            // evaluation, and the kernels hold up to seven VGPRs more)
            if constexpr (kLanesStore) __builtin_amdgcn_sched_barrier(0);
            const double rq_c = (double)st.rq_c, rq_m = (double)st.rq_m;
            TPROF(8);                                                  // state update (readlanes of the signature's request), state store
            // Signature k's byte of the touched node, its block key, summary entries and feasible-node counter (lane-local k).
            auto refresh_sig = [&](int k, bool valid, unsigned nb_raw,
                                   RowRef bytek, const uint4 Tk, const uint2 Fk, unsigned old, unsigned snk, int dirty_bit) {
                const unsigned nb = old ? nb_raw : 0u;                    // static mask / monotone infeasibility
                // One wave: its vector memory accesses are served in order, so the next cycle's loads of this row / state
                // observe these stores; no cache maintenance, no wait.
                if (valid && nb != old) {
                    byte_at(bytek, pos) = (unsigned char)nb;
                    const unsigned m = block_key16_patched<kStraight>(Tk, nb, pos, selA, selB, pos_c, c15);
                    const unsigned e16 = (m >> 4) ? m + (snk << 4) : 0u;
                    if constexpr (COARSE) {
                        // per-16 entry to the workspace; the entry of the 64 positions = max over its four per-16 entries, each
                        // re-keyed to total << 6 | 63 - position (a feasible entry is >= 64, the constants alone stay below)
                        const int j = blk & 3;                            // uniform
                        g_fine[((unsigned)(pstar >> 6) * (unsigned)K + (unsigned)k) * 4u + (unsigned)j] = (unsigned short)e16;
                        const unsigned keep = (j & 1) ? 0x0000FFFFu : 0xFFFF0000u, ins = e16 << ((j & 1) * 16);
                        const unsigned fx = (j & 2) ? Fk.x : ((Fk.x & keep) | ins);
                        const unsigned fy = (j & 2) ? ((Fk.y & keep) | ins) : Fk.y;
                        const unsigned cx = (((fx & 0xFFF0FFF0u) << 2) | (fx & 0x000F000Fu)) | 0x00200030u;
                        const unsigned cy = (((fy & 0xFFF0FFF0u) << 2) | (fy & 0x000F000Fu)) | 0x00000010u;
                        const unsigned mm = pkmax_t(cx, cy);
                        const unsigned c64 = max(mm & 0xFFFFu, mm >> 16);
                        s_sum[k * nbp + (pstar >> 6)] = (unsigned short)(c64 >= 64u ? c64 : 0u);
                    } else {
                        s_sum[k * nbp + blk] = (unsigned short)e16;
                    }
                    if constexpr (!kEager)                                // (kEager: counted down and re-based behind the refresh, see there)
                    if (!nb) {                                            // the node stopped being feasible for this signature
                        const int cidx = k * Cn + dstar;
                        int left;
                        // plain read-modify-write (lane-local: a (signature, class) counter belongs to the lane that owns the signature):
                        // an atomic is performed in L2 and would leave the wave's later plain loads of the counter to a stale L1 line
                        if constexpr (!CNT_LDS) { left = g_cnt[cidx] - 1; g_cnt[cidx] = left; }
                        else { left = s_cnt[cidx] - 1; s_cnt[cidx] = left; }
                        // The class term of row k changes: re-base before its next use -- unless (kCls4: hundreds of small classes, each leaving the
                        // feasible set of every signature at some point) the class that left sat strictly INSIDE the extremes of the last re-base:
                        // lo and hi are then attained by classes that stay, the min-max normalisation (simon.go:76-101) of every other class is
                        // what it was, and the leaver's own entries are all 0 and stay 0 (bytes never come back).  While a row is dirty the stored
                        // extremes may be stale -- it is re-based before its next use whatever this test says.  Static score tables have maxima
                        // of their own: with them every leave re-bases.
                        bool rebase = left == 0;
                        if constexpr (kCls4) {
                            if (rebase && !(sc.static_tables & kStClassTerms)) {
                                const int raw = simon_raw[((KQ > 1 && dirty_bit == KQ - 1) ? my_tc[KQ - 1] : my_tc[0]) * Cn + dstar];
                                const int2 e = s_ext[k];
                                rebase = !(e.x < raw && raw < e.y);
                            }
                        }
                        if (rebase) my_dirty |= 1u << dirty_bit;
#ifdef SIMON_TABLE_DEBUG
                        printf("DBG s=%d step=%d CNT k=%d class=%d left=%d\n", s, i0 + il, k, dstar, left);
#endif
                    }
                }
            };
            // NodeResourcesFit + LeastAllocated + BalancedAllocation of the touched node per signature of this lane.  With 65 .. 128
            // signatures the host puts a signature's twin -- same request, another table class (static mask / Simon row) -- 64 slots up
            // whenever every upper signature has one (TableScalars::static_tables & kStTwins): the upper byte is the lower lane's, unmasked.
            unsigned nbq[KQ];
            // (kLanesStore: without the store's region between them and the refresh, the compiler sinks the selectors' scalar load and the class terms'
            // LDS read into the refresh's region, where the wave waits for each in turn; read here, they stay issued ahead of the state's wait)
            if constexpr (kLanesStore) {
#pragma unroll
                for (int q = 0; q < KQ; ++q) asm volatile("" : : "v"(snq[q]), "s"(selA.x), "s"(selB.x));
            }
            // Round 14 (kFitMask: one-level layout, re-base at the event, no folds): the evaluation hands out its value and its fit apart, the fit as a mask
            // of the wave (every lane is active here), and what the refresh and the re-base ask is scalar logic on SGPR pairs -- the new byte is ONE select on
            // fit & (old != 0), the lanes that refresh are valid & (old != 0) (a byte that comes out as it was is stored again: same byte, same entry;
            // the `nb != old` of the others is a compare per cycle), and "a byte dropped to 0" is (old != 0) & ~fit, formed HERE, in the block of the
            // compares: asked for behind the refresh's region, a flag is materialised per lane and compared again.  The compare of the old byte is the
            // only vector instruction the three cost.  A byte that is 0 stays 0 (static mask, monotone infeasibility) and is not counted as gone.
            unsigned long long goneq[KQ];                              // (kFitMask only)
            if constexpr (kFitMask) {
                NodeEval ev[KQ];
                unsigned long long fitq[KQ];
                ev[0] = eval_node_fit(my_req_c[0], my_req_m[0], my_nz_c[0], my_nz_m[0], my_zero[0], rq_c, rq_m, nzc, nzm, (int)st.freep, sh);
                fitq[0] = fit_mask_t(ev[0], free_m, zero_m[0]);
                if constexpr (KQ > 1) {
                    if (sc.static_tables & kStTwins) { ev[KQ - 1] = ev[0]; fitq[KQ - 1] = fitq[0]; }   // the twin takes the one evaluation's value and mask
                    else {
                        ev[KQ - 1] = eval_node_fit(my_req_c[KQ - 1], my_req_m[KQ - 1], my_nz_c[KQ - 1], my_nz_m[KQ - 1], my_zero[KQ - 1], rq_c, rq_m, nzc, nzm, (int)st.freep, sh);
                        fitq[KQ - 1] = fit_mask_t(ev[KQ - 1], free_m, zero_m[KQ - 1]);
                    }
                }
                unsigned long long oldm[KQ];
#pragma unroll
                for (int q = 0; q < KQ; ++q) {
                    oldm[q] = __ballot(oldq[q] != 0u);
                    goneq[q] = oldm[q] & ~fitq[q];
                }
#pragma unroll
                for (int q = 0; q < KQ; ++q) {
                    nbq[q] = __builtin_amdgcn_inverse_ballot_w64(fitq[q] & oldm[q]) ? ev[q].val : 0u;
                    if (__builtin_amdgcn_inverse_ballot_w64(kvalid_m[q] & oldm[q])) {
                        byte_at(bytep[q], pos) = (unsigned char)nbq[q];
                        const unsigned m = block_key16_patched<kStraight>(T[q], nbq[q], pos, selA, selB, pos_c, c15);
                        s_sum[kk[q] * nbp + blk] = (unsigned short)((m >> 4) ? m + (snq[q] << 4) : 0u);
                    }
                }
            } else {
                nbq[0] = eval_node(my_req_c[0], my_req_m[0], my_nz_c[0], my_nz_m[0], my_zero[0], rq_c, rq_m, nzc, nzm, (int)st.freep, sh);
                if constexpr (KQ > 1) {
                    if (sc.static_tables & kStTwins) nbq[KQ - 1] = nbq[0];
                    else nbq[KQ - 1] = eval_node(my_req_c[KQ - 1], my_req_m[KQ - 1], my_nz_c[KQ - 1], my_nz_m[KQ - 1], my_zero[KQ - 1], rq_c, rq_m, nzc, nzm, (int)st.freep, sh);
                }
                if constexpr (kFoldable) {
                    if (__builtin_expect(fold, 0)) {                      // folded exclusions: the signatures this landing rules out get byte 0
#pragma unroll
                        for (int q = 0; q < KQ; ++q) nbq[q] = ((xfold[q] >> (kk[q] & 31)) & 1u) ? 0u : nbq[q];
                    }
                }
            }
            unsigned gu[8] = {0, 0, 0, 0, 0, 0, 0, 0};                   // GPU fold: the landing node's devices after Reserve (MANY: the further groups read them)
            bool gbooked = false;
            if constexpr (kGpuFoldable) {
                if (__builtin_expect(gfold, 0)) {
                    // Open-Gpu-Share folded into the table: a GPU pod the scheduler placed books its devices (Reserve,
                    // open-gpu-share.go:147-188: every lane alike), and the GPU signatures whose request stopped fitting the node get
                    // byte 0 -- for good (device memory is never released).  Pods bound by Spec.NodeName never reach Reserve.
                    unsigned greq = (unsigned)(hiq ? __builtin_amdgcn_readlane((int)my_greq[KQ - 1], sl) : __builtin_amdgcn_readlane((int)my_greq[0], sl));
                    int gnum = hiq ? __builtin_amdgcn_readlane(my_gnum[KQ - 1], sl) : __builtin_amdgcn_readlane(my_gnum[0], sl);
                    if (MANY && __builtin_expect(r_sig >= 64 * KQ, 0)) {   // a signature beyond the register-resident ones: its row (uniform index)
                        const SigRow rs = sigs[r_sig];
                        greq = (unsigned)rs.pad[0]; gnum = rs.pad[1];
                    }
                    if (gnum > 0 && !bound) {
                        unsigned (&u)[8] = gu;
                        u[0] = gfa.x; u[1] = gfa.y; u[2] = gfa.z; u[3] = gfa.w; u[4] = gfb.x; u[5] = gfb.y; u[6] = gfb.z; u[7] = gfb.w;
                        gbooked = true;
                        const unsigned long long booked = gpu_commit_t(u, gfc, gft, greq, gnum);
                        if (sc.static_tables & kStGpuSlices) {                       // the caller wants the devices (simon_batch_out.gpu_slices), by pod id
                            const int pid = __builtin_amdgcn_readfirstlane(order[i0 + il]);
                            if (lane == 0) gp(cold->gpu_slices)[(size_t)s * (size_t)P + (size_t)pid] = booked;
                        }
                        if (lane == 0) {
                            *(uint4*)(g_fu + (size_t)pstar * 8) = make_uint4(u[0], u[1], u[2], u[3]);
                            *(uint4*)(g_fu + (size_t)pstar * 8 + 4) = make_uint4(u[4], u[5], u[6], u[7]);
                        }
#pragma unroll
                        for (int q = 0; q < KQ; ++q)
                            if (my_gnum[q] != 0 && !gpu_fits_t(u, gfc, gft, my_greq[q], my_gnum[q])) nbq[q] = 0u;
                    }
                }
            }
            if constexpr (!kFitMask) {                                 // (kFitMask: refreshed above)
#pragma unroll
                for (int q = 0; q < KQ; ++q)
                    refresh_sig(kk[q], kvalid[q], nbq[q], bytep[q], T[q], COARSE ? F[q] : make_uint2(0u, 0u),
                                oldq[q], snq[q], q);
            }
            if constexpr (kEager) {
                // The node stopped being feasible for some signature (one uniform test where the lanes' own regions stood): the lanes count their
                // (signature, class) down, lane-local as ever, and every row whose counter reached 0 -- the class left the signature's feasible set, its
                // class terms change -- is re-based here, at the event, by the whole wave: renormalise is a function of the counters alone and they only
                // fall, so the row's next use finds what a re-base at that use would have written, and the plain pod asks nothing before its scan.
                // The test: bytes, so old > new << 8 iff new == 0 < old -- ONE compare per signature, and a byte that was 0 stays 0 whatever the evaluation
                // says.  A lane beyond K works on signature 0's row and is not masked out here (the and with kvalid made the compiler materialise the flag: a
                // v_cndmask and a second compare per cycle): at worst it sends the wave into the rare block for nothing -- the counters below ask kvalid.
                bool gone = false;
#pragma unroll
                for (int q = 0; q < KQ; ++q) gone |= oldq[q] > (nbq[q] << 8);
                // (kFitMask: the uniform test is the masks' own, (old != 0) & ~fit from above, and costs no vector instruction -- the compares of `gone` are
                // dead there; the rare block's per-lane test reads the bytes as ever: the new byte is 0 exactly where the fit failed)
                bool any_gone;
                if constexpr (kFitMask) {
                    unsigned long long gone_m = 0ull;
#pragma unroll
                    for (int q = 0; q < KQ; ++q) gone_m |= goneq[q];
                    any_gone = gone_m != 0ull;
                } else any_gone = __ballot(gone) != 0ull;
                if (__builtin_expect(any_gone, 0)) {
                    unsigned long long emptied[KQ];
#pragma unroll
                    for (int q = 0; q < KQ; ++q) {
                        bool last = false;
                        if (kvalid[q] && oldq[q] > (nbq[q] << 8)) {
                            // plain read-modify-write (a (signature, class) counter belongs to the lane that owns the signature): an atomic is
                            // performed in L2 and would leave the wave's later plain loads of the counter to a stale L1 line
                            const int cidx = kk[q] * Cn + dstar;
                            int left;
                            if constexpr (!CNT_LDS) { left = g_cnt[cidx] - 1; g_cnt[cidx] = left; }
                            else { left = s_cnt[cidx] - 1; s_cnt[cidx] = left; }
                            last = left == 0;
#ifdef SIMON_TABLE_DEBUG
                            printf("DBG s=%d step=%d CNT k=%d class=%d left=%d\n", s, i0 + il, kk[q], dstar, left);
#endif
                        }
                        emptied[q] = __ballot(last);
                    }
#pragma unroll
                    for (int q = 0; q < KQ; ++q) {
                        for (unsigned long long m = emptied[q]; m; m &= m - 1) {
                            const int k = 64 * q + __builtin_ctzll(m);
                            renormalise(k, sig_class(k));
                        }
                    }
                }
            }
            // MANY: the further groups (their table rows arrived with group 0's; the signature rows of TableCold::sigs are L2-hot)
            if constexpr (MANY) {
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    if (128 * (g + 1) < K) {
                        SigRow rg[KQ];
                        unsigned sng[KQ];
#pragma unroll
                        for (int q = 0; q < KQ; ++q) { rg[q] = sigs[kg[g][q]]; sng[q] = s_sn[kg[g][q] * Cn + dstar]; }
#pragma unroll
                        for (int q = 0; q < KQ; ++q)
                            refresh_sig(kg[g][q], 128 * (g + 1) + 64 * q + lane < K,
                                        ((fold && ((xfg[g][q] >> (kg[g][q] & 31)) & 1u)) ||
                                         (kGpuFoldable && gbooked && rg[q].pad[1] != 0 && !gpu_fits_t(gu, gfc, gft, (unsigned)rg[q].pad[0], rg[q].pad[1]))) ? 0u :
                                        eval_node(rg[q].req_c, rg[q].req_m, rg[q].nz_c, rg[q].nz_m, rg[q].flags & 1u, rq_c, rq_m, nzc, nzm, (int)st.freep, sh),
                                        rowg[g][q], Tg[g][q], Fg[g][q], oldg[g][q], sng[q], 2 * (g + 1) + q);
                    }
                }
                // 385 .. 1 023 signatures (round 4): the groups beyond the two whose rows travel with group 0's take a round trip of their
                // own each -- a problem of that many signatures that needs generation 7's walks or a fold has the all-feature kernel as
                // its alternative, not a faster table.  (uniform trip count; a lane beyond K evaluates signature 0 and stores nothing)
                for (int g = NG; 128 * (g + 1) < K; ++g) {
#pragma unroll
                    for (int q = 0; q < KQ; ++q) {
                        const int kq = 128 * (g + 1) + 64 * q + lane;
                        const int kx = kq < K ? kq : 0;
                        const RowRef rowx = row_ref(tile_blk((unsigned)(pstar >> 4)) + (unsigned)kx * KS);
                        const uint4 Tx = row_vec(rowx);
                        const unsigned oldx = row_byte(rowx, pstar & 15);
                        const uint2 Fx = *(const uint2*)(g_fine + ((unsigned)(pstar >> 6) * (unsigned)K + (unsigned)kx) * 4u);
                        const unsigned xfx = fold ? gp(cold->foldx)[(unsigned)r_sig * KW + ((unsigned)kx >> 5)] : 0u;
                        const SigRow rx = sigs[kx];
                        const unsigned snx = s_sn[kx * Cn + dstar];
                        refresh_sig(kx, kq < K,
                                    ((fold && ((xfx >> (kx & 31)) & 1u)) ||
                                     (kGpuFoldable && gbooked && rx.pad[1] != 0 && !gpu_fits_t(gu, gfc, gft, (unsigned)rx.pad[0], rx.pad[1]))) ? 0u :
                                    eval_node(rx.req_c, rx.req_m, rx.nz_c, rx.nz_m, rx.flags & 1u, rq_c, rq_m, nzc, nzm, (int)st.freep, sh),
                                    rowx, Tx, Fx, oldx, snx, 2 * (g + 1) + q);
                    }
                }
            }
            TPROF(9);                                                  // evaluation, patch, block key, summary / table stores
            if (REST && __builtin_expect(rw != 0, 0)) rest_assume_store(RL, pstar, r_nrows, rowv, bound ? -1 : r_gs, r_xs, i0 + il);
            if (SPREAD && sp_match != 0) spread_count_store(SPL, pstar, dstar, spv, spt, sp_soft, sp_match);
            TPROF(19);                                                 // spread: counter stores
            __builtin_amdgcn_wave_barrier();
            TPROF(6);                                                  // REST: term rows, GPU commit and GPU rows
