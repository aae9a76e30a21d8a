// Body of one output tile of the ping-pong NT block (csrc/gemm_nt_pp.h includes it twice: as the body of gemm_nt_pp_kernel and, ACG = 2,
// as the tile function of gemm_nt_pp_far_kernel - the same text, so that the kernel every step runs is compiled exactly as before).
// In scope: template arguments ELEM, EPI, ACG, SEG; const NtParams& p; char* smem; int far_tm, far_tn (ACG = 2: the tile to compute);
// constexpr int AROWS (gemm_nt_pp_rows_kernel: 1 = row m of A is row p.gather[m] of p.A - a row table, plain rows of C; ACG = SEG = 0).
    constexpr int HT = 16384;                        // half-tile bytes; slot = parity*4 + kind, kind 0 A0, 1 B0, 2 B1, 3 A1
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 2, wc = wid & 3;
    int tm, tn;
    if constexpr (ACG == 2) {
        tm = far_tm; tn = far_tn;
    } else if constexpr (SEG) {   // XCD patches of 16 M tiles x (slot, both channel halves): 7.37 against 7.50 ms for 4 x 8
        xcd_patch_map(blockIdx.x, p.tiles_m, p.tiles_n, tm, tn, 16, 2);
    } else if (p.patch_aligned) {
        if (!xcd_patch_map_aligned(blockIdx.x, p.tiles_m, p.tiles_n, tm, tn)) return;  // padding block (uniform exit)
    } else {
        xcd_patch_map(blockIdx.x, p.tiles_m, p.tiles_n, tm, tn);
    }
    const int m0 = tm * 256;
    int n0 = tn * 256, n_tile = tn, Kloc = p.K, seg_py = 0, seg_px = 0, seg_ny = 1, seg_nx = 1, seg_c0 = 0;
    long ldb = p.ldb, b_off = 0;
    if constexpr (SEG) {
        // virtual N tile = (slot, channel half).  Slots are the 16 patch pixels pp in natural order; with p.seg_split the four centre pixels
        // (4 combinations, K = 4096) take TWO slots of 2 combinations each, summed by the reader (windows_patch_sum): the blocks of an XCD
        // patch share their A and B tiles through the L2 only while they stay at the same K step, and blocks of 64 K steps drift apart
        // (measured: slots ordered by class, i.e. whole patches of K = 4096 blocks, 10.9 ms per launch against 8.6 in natural order).
        const int slot = tn >> 1;
        int pp = 0, part = 0;
        if (p.seg_split) {
            int acc = 0;
            for (pp = 0; pp < 16; ++pp) {
                const int wdt = (((pp >> 2) == 1 || (pp >> 2) == 2) && ((pp & 3) == 1 || (pp & 3) == 2)) ? 2 : 1;
                if (slot < acc + wdt) { part = slot - acc; break; }
                acc += wdt;
            }
        } else {
            pp = slot;
        }
        n_tile = tn & 1;
        n0 = slot * 512 + n_tile * 256;                // output columns: slot, channel half
        seg_py = pp >> 2; seg_px = pp & 3;
        auto cnt1 = [](int c) { return (c == 0 || c == 3) ? 1 : 2; };
        seg_ny = cnt1(seg_py); seg_nx = cnt1(seg_px);
        const int ncomb = seg_ny * seg_nx;
        seg_c0 = (p.seg_split && ncomb == 4) ? 2 * part : 0;
        Kloc = ((p.seg_split && ncomb == 4) ? 2 : ncomb) * 1024;
        ldb = ncomb * 1024 + p.seg_bpad;               // row of B_pp: all combinations of pp (+ padding)
        for (int j = 0; j < pp; ++j) b_off += 512L * (1024 * (cnt1(j >> 2) * cnt1(j & 3)) + p.seg_bpad);     // B_pp follows B_0 .. B_pp-1
        b_off += seg_c0 * 1024;
    }
    int Mlim = p.M;
    long img0 = 0;
    if constexpr (ACG) {
        Mlim = min(p.M, 4 * *p.gather_n);
        if (m0 >= Mlim) return;                      // the grid is sized for the bound (uniform exit, before any barrier)
        img0 = p.gather[m0 >> 2] >> (2 * p.lgS - 2);       // windows per map: (S/2)^2
    }
    const int SP = (1 << p.lgS) + 2;                  // padded map side (ACG only)
    const long img_elems = (long)SP * SP * p.Cin;

    // ---- staging sources: wave w writes LDS rows (2w+q)*8 .. +7 of every half tile (q = 0,1), 8 lanes per 128-B row
    const int lrow = lane >> 3, cpos = lane & 7;
    const u16* const a_blk = ACG ? p.A + img0 * img_elems : (AROWS ? p.A : p.A + (long)m0 * p.lda);
    const u16* const b_blk = p.B + b_off + (long)(n_tile * 256) * ldb + (p.tile_group ? (long)p.tile_group[tm] * p.group_stride : 0L);
    int voff[4][2];                                  // byte offsets from a_blk / b_blk
    int far_map[4][2] = {};                          // ACG = 2: maps of the two list entries (lanes 0-31 / 32-63) behind A load 2h + q
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int r = (wid * 2 + q) * 8 + lrow;
        const int chunk = (cpos ^ ((r >> 1) & 7)) << 3;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int m = (r >> 6) * 128 + h * 64 + (r & 63);
            if (m0 + m > Mlim - 1) m = Mlim - 1 - m0;
            if constexpr (ACG) {
                const int mg = m0 + m;
                const int mv = p.gather[mg >> 2] * 4 + (mg & 3);
                if constexpr (ACG == 2) {            // offset inside the row's own map
                    const int mp = mv >> (2 * p.lgS);
                    voff[h ? 3 : 0][q] = (int)((conv_row_base(mv, p.lgS, p.Cin) - mp * img_elems + chunk) * 2);
                    far_map[2 * h + q][0] = __builtin_amdgcn_readlane(mp, 0);
                    far_map[2 * h + q][1] = __builtin_amdgcn_readlane(mp, 32);
                } else
                voff[h ? 3 : 0][q] = (int)((conv_row_base(mv, p.lgS, p.Cin) - img0 * img_elems + chunk) * 2);
            } else if constexpr (AROWS) {              // source rows below 2^31 bytes from p.A (checked by the entry point)
                voff[h ? 3 : 0][q] = (int)((p.gather[m0 + m] * p.lda + chunk) * 2);
            } else {
                voff[h ? 3 : 0][q] = (int)((m * p.lda + chunk) * 2);
            }
            const int n = (r >> 5) * 64 + h * 32 + (r & 31);
            voff[1 + h][q] = (int)((n * ldb + chunk) * 2);
        }
    }
    auto stage = [&](int kind, int t) __attribute__((always_inline)) {
        char* base = smem + (((t & 1) << 2) + kind) * HT + wid * 2048;
        const u16* g = (kind == 0 || kind == 3) ? a_blk : b_blk;
        int soff = t << 7;
        if constexpr (ACG) {
            if (kind == 0 || kind == 3) {            // K tile t = (64-channel chunk t/9, tap t%9) of the padded 18x18 map
                const int cc = t / 9, tap = t - cc * 9;
                const int ky = tap / 3, kx = tap - 3 * ky;
                soff = ((ky * SP + kx) * p.Cin + (cc << 6)) * 2;
                if constexpr (ACG == 2) {
#pragma unroll
                    for (int q = 0; q < 2; ++q) {    // one descriptor per list entry: each half of the wave loads under its own
                        const int* fm = far_map[(kind ? 2 : 0) + q];
#pragma unroll
                        for (int s = 0; s < 2; ++s)
                            if ((lane >> 5) == s) buf_load_lds16(p.A + fm[s] * img_elems, voff[kind][q], soff, base + q * 1024);
                    }
                    return;
                }
            }
        }
        if constexpr (SEG) {
            if (kind == 0 || kind == 3) {            // K tile t: combination c = t / 16 -> own pixel (qy, qx) of the window, channels (t % 16) * 64
                const int c = seg_c0 + (t >> 4);
                const int cy = seg_nx == 2 ? (c >> 1) : c, cx = seg_nx == 2 ? (c & 1) : 0;
                const int qy = seg_ny == 1 ? (seg_py == 3) : cy, qx = seg_nx == 1 ? (seg_px == 3) : cx;
                g = a_blk + (long)(qy * 2 + qx) * p.seg_stride;       // wave-uniform: goes into the buffer descriptor
                soff = (t & 15) << 7;
            }
        }
        if constexpr (AROWS) {
            if (kind == 0 || kind == 3) {            // offsets reach the last bytes below 2 GiB
                buf_load_lds16_2g(g, voff[kind][0], soff, base);
                buf_load_lds16_2g(g, voff[kind][1], soff, base + 1024);
                return;
            }
        }
        buf_load_lds16(g, voff[kind][0], soff, base);
        buf_load_lds16(g, voff[kind][1], soff, base + 1024);
    };

    // ---- fragment reads: 16 rows x 32 k per instruction step, two steps per K tile.  Lane l reads row l&15 of the fragment, logical chunk
    // 4*ks + (l>>4) (row swizzle (row>>1)&7 only depends on lane&15: fragments start at multiples of 16 rows)
    const int l15 = lane & 15, kg = lane >> 4, sw = (l15 >> 1) & 7;
    int ko[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) ko[ks] = ((ks * 4 + kg) ^ sw) << 4;
    const int a_rd = (wr * 64 + l15) * 128, b_rd = (wc * 32 + l15) * 128;
    s16x8 af[4][2], bf[4][2];
    auto read_a = [&](int h, int par) __attribute__((always_inline)) {
        const char* base = smem + ((par << 2) + (h ? 3 : 0)) * HT + a_rd;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) af[i][ks] = *reinterpret_cast<const s16x8*>(base + i * 2048 + ko[ks]);
    };
    auto read_b = [&](int par) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {                  // column fragment j of the wave: b-half j>>1, its rows (j&1)*16 .. +15
            const char* base = smem + ((par << 2) + 1 + (j >> 1)) * HT + b_rd + (j & 1) * 2048;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) bf[j][ks] = *reinterpret_cast<const s16x8*>(base + ko[ks]);
        }
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;
    auto half = [&](int a) __attribute__((always_inline)) {       // k step outermost: every accumulator sees its K groups in increasing k
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (EPI == EPI_STORE_F32T) acc[4 * a + i][j] = mfma16<ELEM>(bf[j][ks], af[i][ks], acc[4 * a + i][j]);
                    else acc[4 * a + i][j] = mfma16<ELEM>(af[i][ks], bf[j][ks], acc[4 * a + i][j]);
                }
        SGC_PP_BARRIER();
    };
    // end of a load section: counted wait for the half tiles the NEXT phase reads, retire this phase's reads, barrier
#define SGC_PP_CLOSE(STEADY)                                   \
    do {                                                       \
        if (STEADY) SGC_WAIT_VM(8); else SGC_WAIT_VM(0);       \
        SGC_WAIT_LGKM0();                                      \
        SGC_PP_BARRIER();                                      \
    } while (0)

    const int nk = Kloc >> 6;
    // ---- prologue: ring order is [A0 B0 B1](t) in phase Y(t-2), A1(t) in phase X(t-1)
    stage(0, 0); stage(1, 0); stage(2, 0); stage(3, 0);
    if (nk > 1) { stage(0, 1); stage(1, 1); stage(2, 1); if constexpr (ACG == 2) SGC_WAIT_VM(0); else SGC_WAIT_VM(8); } else SGC_WAIT_VM(0);
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();        // wave row 1 runs one barrier slot behind wave row 0

    auto tile = [&](int t, int par, auto steady_c) __attribute__((always_inline)) {
        constexpr bool STEADY = decltype(steady_c)::value;       // tile t+2 exists
        read_a(0, par); read_b(par);                             // phase X
        if (t + 1 < nk) stage(3, t + 1);                         // A1(t+1) replaces A1(t-1), read in phase Y(t-1)
        SGC_PP_CLOSE(STEADY && ACG != 2);
        half(0);
        read_a(1, par);                                          // phase Y
        if (STEADY) { stage(0, t + 2); stage(1, t + 2); stage(2, t + 2); }     // replace what phase X(t) read
        SGC_PP_CLOSE(STEADY && ACG != 2);
        half(1);
    };
    int t = 0;
#pragma unroll 1
    for (; t + 2 < nk; ++t) tile(t, t & 1, std::true_type{});
#pragma unroll 1
    for (; t < nk; ++t) tile(t, t & 1, std::false_type{});
    if (wr == 0) __builtin_amdgcn_s_barrier();        // re-align the two wave rows

    bool stored = false;
    if constexpr (EPI == EPI_STORE && !ACG) {         // (gathered rows are scattered: the generic epilogue)
        if (p.epi_lds) { nt_epilogue_store16<ELEM>(p, acc, m0, n0, wr, wc, lane, wid, smem); stored = true; }
    }
    if constexpr (EPI == EPI_RELUMASK && !ACG) {
        if (p.epi_lds && !p.bias && (p.ldc & 7) == 0) { nt_epilogue_store16<ELEM, true>(p, acc, m0, n0, wr, wc, lane, wid, smem); stored = true; }
    }
    if (stored) {
    } else if constexpr (EPI == EPI_STORE_F32T) {
        static_assert(!ACG, "transposed f32 tile: plain rows only");
        nt_epilogue_f32t(p, acc, m0, n0, wr, wc, lane);
    }
    else if constexpr (ACG && EPI == EPI_POOL) {
        if (p.epi_lds) nt_epilogue_pool16<ELEM, true>(p, acc, m0, n0, wr, wc, lane, wid, smem, Mlim);
        else nt_epilogue<ELEM, EPI, 8, 4, true>(p, acc, m0, n0, wr, wc, lane, Mlim);
    }
    else if constexpr (ACG) nt_epilogue<ELEM, EPI, 8, 4, true>(p, acc, m0, n0, wr, wc, lane, Mlim);
    else nt_epilogue<ELEM, EPI, 8, 4>(p, acc, m0, n0, wr, wc, lane);
