// Body of the ping-pong TN block (csrc/gemm_tn.h includes it twice: as the body of gemm_tn_pp_kernel and, AROWS = 1, of
// gemm_tn_pp_rows_kernel - the same text, so that the kernels every step runs compile exactly as before).
// In scope: template arguments ELEM, BMODE, ACONV; constexpr int AROWS; const TnParams p; char smem[].
    static_assert(!AROWS || (BMODE == BMODE_PLAIN && !ACONV), "row table: plain operands only");
    constexpr int HT = 16384, BM = 256, BN = 256;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 2, wc = wid & 3;
    const int tiles = p.tiles_n * p.tiles_m;
    int split, tm, tn;
    if (p.xcd_map) {
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        split = j / 9;
        tm = xcd & 3;
        tn = (j - split * 9) * 2 + (xcd >> 2);
    } else {
        split = blockIdx.x / tiles;
        if (p.xcd_patch) xcd_patch_map(blockIdx.x - split * tiles, p.tiles_m, p.tiles_n, tm, tn);
        else supertile_map(blockIdx.x - split * tiles, p.tiles_m, p.tiles_n, tm, tn);
    }
    const int m0 = tm * BM, n0 = tn * BN;
    int kt_begin = split * p.ktiles_per_split;
    int kt_end = kt_begin + p.ktiles_per_split;
    const int nk_total = p.K >> 6;
    if (kt_end > nk_total) kt_end = nk_total;
    if (p.goff) { kt_begin = p.goff[split] >> 6; kt_end = p.goff[split + 1] >> 6; }      // grouped: "split" is the group
    const int nk = kt_end - kt_begin;

    // ---- staging: one instruction = one k block (4 rows) x 8 sub-blocks of a half tile; wave w owns k blocks 2w, 2w+1
    const int kr = (lane >> 1) & 3, sb = lane >> 3, c8 = (lane & 1) * 8;
    int voff[4][2];                                  // kind 0 A0, 1 B0, 2 B1, 3 A1: byte offsets inside a K tile
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int kl = (wid * 2 + q) * 4 + kr;
        long arow;
        if constexpr (ACONV) arow = conv_row_base(kl, p.lgS, p.CinA) + (long)((1 << p.lgS) + 3) * p.CinA;
        else if constexpr (AROWS) arow = 0;          // the row comes from the table, per K tile (rows_of below)
        else arow = (long)kl * p.lda;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            voff[h ? 3 : 0][q] = (int)((arow + m0 + ((sb >> 2) * 8 + h * 4 + (sb & 3)) * 16 + c8) * 2);
            const int col = n0 + ((sb >> 1) * 4 + h * 2 + (sb & 1)) * 16;      // first column of this lane's 16-column sub-block
            long b;
            if constexpr (BMODE == BMODE_CONV) {
                // the tap is a per-lane quantity: with Cin = 128 a 256-column tile spans two taps, and the last tile of
                // N = 9*Cin may reach past tap 8 (those columns read tap 8 again and are never stored)
                const int tap_raw = col / p.Cin;
                const int tap = tap_raw > 8 ? 8 : tap_raw;
                const int ky = tap / 3, kx = tap - 3 * ky;
                b = conv_row_base(kl, p.lgS, p.Cin) + (long)(ky * ((1 << p.lgS) + 2) + kx) * p.Cin + (col - tap_raw * p.Cin);
            } else if constexpr (BMODE == BMODE_GATHER) {
                const int tap_raw = col / p.Cin;
                const int tap = tap_raw > 8 ? 8 : tap_raw;
                const int ky = tap / 3, kx = tap - 3 * ky;
                // pixel kr of the window + tap + column; the window's own offset is added per K tile (stage)
                b = (long)(((kr >> 1) + ky) * 18 + (kr & 1) + kx) * p.Cin + (col - tap_raw * p.Cin);
            } else if constexpr (BMODE == BMODE_PATCH) {
                const int tap_raw = col / p.Cin;
                const int tap = tap_raw > 8 ? 8 : tap_raw;
                const int ky = tap / 3, kx = tap - 3 * ky;
                b = (long)((kl >> 2) * 16 + ((kr >> 1) + ky) * 4 + (kr & 1) + kx) * p.Cin + (col - tap_raw * p.Cin);
            } else {
                b = (long)kl * p.ldb + col;
            }
            voff[1 + h][q] = (int)((b + c8) * 2);
        }
    }
    // ---- AROWS: the table entries of the wave's two k blocks of one K tile (wave-uniform), and the lane's two source rows as byte offsets
    // The table is read through the constant address space (nothing writes it while the kernel runs) at a wave-uniform index: four
    // consecutive scalar words = one 16-byte scalar load, no vector memory instruction (the counted vmcnt waits stay what they are).
    int row_quad[2][4] = {};
    int row_off[2] = {0, 0};
    auto rows_fetch = [&](int it) __attribute__((always_inline)) {           // K tile it of this split, held to its last one (inside the table)
        const int kt = kt_begin + min(it, nk - 1);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const auto* te = (const __attribute__((address_space(4))) int*)(p.gather) + __builtin_amdgcn_readfirstlane(kt * 64 + (wid * 2 + q) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) row_quad[q][j] = te[j];
        }
    };
    auto rows_select = [&]() __attribute__((always_inline)) {
        const int pitch = (int)(p.lda * 2);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int lo = (kr & 1) ? row_quad[q][1] : row_quad[q][0], hi = (kr & 1) ? row_quad[q][3] : row_quad[q][2];
            row_off[q] = ((kr & 2) ? hi : lo) * pitch;
        }
    };
    auto stage = [&](int kind, int it) __attribute__((always_inline)) {      // it = K tile index inside this split
        char* base = smem + (((it & 1) << 2) + kind) * HT + wid * 2048;
        if constexpr (AROWS) {
            if (kind == 0 || kind == 3) {            // rows of K tile ``it`` are in row_off (rows_select ran on its table entries)
                buf_load_lds16_2g(p.A, voff[kind][0] + row_off[0], 0, base);       // (offsets reach the last bytes below 2 GiB)
                buf_load_lds16_2g(p.A, voff[kind][1] + row_off[1], 0, base + 1024);
                return;
            }
        }
        const int kt = kt_begin + it;
        long toff;
        const u16* g;
        if (kind == 0 || kind == 3) {
            if constexpr (ACONV) toff = conv_row_base(kt * 64, p.lgS, p.CinA); else toff = (long)kt * 64 * p.lda;
            g = p.A + toff;                          // wave-uniform: goes into the buffer descriptor
        } else {
            if constexpr (BMODE == BMODE_CONV) toff = conv_row_base(kt * 64, p.lgS, p.Cin);
            else if constexpr (BMODE == BMODE_PATCH) toff = (long)kt * 16 * 16 * p.Cin;        // 16 windows per K tile, 16 patch pixels each
            else toff = (long)kt * 64 * p.ldb;
            g = p.B + toff;                          // (BMODE_GATHER: replaced below by the window's own base)
        }
        if constexpr (BMODE == BMODE_GATHER) {
            if (kind == 1 || kind == 2) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int code = __builtin_amdgcn_readfirstlane(p.gather[__builtin_amdgcn_readfirstlane(kt * 16 + wid * 2 + q)]);
                    const int W = code & 63;
                    const u16* gq = p.B + ((long)((code >> 6) * 18 + 2 * (W >> 3)) * 18 + 2 * (W & 7)) * p.Cin;
                    buf_load_lds16(gq, voff[kind][q], 0, base + q * 1024);
                }
                return;
            }
        }
        buf_load_lds16(g, voff[kind][0], 0, base);
        buf_load_lds16(g, voff[kind][1], 0, base + 1024);
    };

    // ---- fragment reads: sub-block (wr*4 + i*2 + g) of an A half, (wc*2 + g) of a B half; k blocks ks*4 + kh*2 (+1)
    const int g = (lane >> 4) & 1, kh = lane >> 5, t16 = lane & 15;
    const int lane_off = (t16 >> 2) * 32 + (t16 & 3) * 8 + kh * 2048;
    const int a_rd = (wr * 4 + g) * 128 + lane_off, b_rd = (wc * 2 + g) * 128 + lane_off;
    s16x8 af[2][4], bf[2][4];
    auto tr2 = [&](const char* ptr) __attribute__((always_inline)) {
        const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(ptr));
        const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(ptr + 1024));
        return __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
    };
    auto read_a = [&](int h, int par) __attribute__((always_inline)) {
        const char* base = smem + ((par << 2) + (h ? 3 : 0)) * HT + a_rd;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) af[i][ks] = tr2(base + i * 256 + ks * 4096);
    };
    auto read_b = [&](int par) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const char* base = smem + ((par << 2) + 1 + h) * HT + b_rd;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) bf[h][ks] = tr2(base + ks * 4096);
        }
    };

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    auto half = [&](int a) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[2 * a + i][j] = mfma32<ELEM>(af[i][ks], bf[j][ks], acc[2 * a + i][j]);
        SGC_PP_BARRIER();
    };

    if (nk > 0) {
        if constexpr (AROWS) { rows_fetch(0); rows_select(); }
        stage(0, 0); stage(1, 0); stage(2, 0); stage(3, 0);
        if (nk > 1) {
            if constexpr (AROWS) { rows_fetch(1); rows_select(); }
            stage(0, 1); stage(1, 1); stage(2, 1);
            if constexpr (AROWS) rows_fetch(2);      // what phase Y of tile 0 selects from
            SGC_WAIT_VM(8);
        } else SGC_WAIT_VM(0);
    }
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();
    // AROWS: row_off holds the rows of tile it + 1 through phase X (A1 of it + 1) and those of tile it + 2 from phase Y on (A0 of it + 2,
    // then A1 in the next tile's phase X); the select stands ahead of the phase's LDS reads, where its wait on the table entries -
    // fetched a whole tile earlier and drained with the last phase - holds nothing back
    auto tile = [&](int it, int par, auto steady_c) __attribute__((always_inline)) {
        constexpr bool STEADY = decltype(steady_c)::value;
        read_a(0, par); read_b(par);
        if (it + 1 < nk) stage(3, it + 1);
        SGC_PP_CLOSE(STEADY);
        half(0);
        if constexpr (AROWS && STEADY) { rows_select(); __builtin_amdgcn_sched_barrier(0); }
        read_a(1, par);
        if (STEADY) { stage(0, it + 2); stage(1, it + 2); stage(2, it + 2); }
        if constexpr (AROWS && STEADY) rows_fetch(it + 3);
        SGC_PP_CLOSE(STEADY);
        half(1);
    };
    int it = 0;
#pragma unroll 1
    for (; it + 2 < nk; ++it) tile(it, it & 1, std::true_type{});
#pragma unroll 1
    for (; it < nk; ++it) tile(it, it & 1, std::false_type{});
    if (wr == 0) __builtin_amdgcn_s_barrier();

    float* C = p.C + (p.goff ? (long)split * p.N : (long)split * p.slab_stride);
    const int hh = lane >> 5, cl = lane & 31;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wc * 64 + j * 32 + cl;
            if (col >= p.N) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wr * 128 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                C[(long)row * p.ldc + col] = acc[i][j][r];
            }
        }
