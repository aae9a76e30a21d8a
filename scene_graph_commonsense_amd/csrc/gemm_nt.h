// NT GEMM for gfx950:  C[M,N] = A[M,K] * B[N,K]^T, 16-bit inputs (f16 or bf16), f32 accumulate on
// v_mfma_f32_16x16x32_{f16,bf16}.  128x128x64 block tile, 4 wavefronts (2x2), each 64x64 = 4x4 MFMA tiles.
//
// THE ACCUMULATION CONTRACT.  Several tests demand bit equality between runs that reach DIFFERENT blocks of this family for the
// same output element (one image group against many, shared against per-pair conv3, conv2 on halves against whole maps): the
// block is chosen by the size of the problem.  They agree because every NT kernel here (gemm_nt_kernel in both block sizes,
// gemm_nt_pp_kernel in all its forms, conv16_halo_pp_kernel)
//   * adds, into each output element, ONE 16x16x32 instruction per 32 consecutive k (lane group l>>4 supplies k = 8*(l>>4) .. +7),
//   * in increasing k of its own K order (plain: k; convolutions: (64-channel chunk, tap, channel)),
//   * and never splits or reorders that sequence (no split-K, no second accumulator per element).
// Which lane or register holds an element, and which operand is passed first, does not enter.  A kernel that joins the family
// keeps all three; the TN (weight gradient) and sparse kernels are compared only among themselves and run 32x32x16.
// Why this shape: at equal instruction cycles per FLOP the launches measured shorter on it than on 32x32x16 (conv3 forward over the
// listed windows -9 %, the step -1.0 ... -1.1 ms); in a counter pass of each build that launch ran +3 % wave cycles at an effective clock of
// 1.53 against 1.41 GHz (GRBM_GUI_ACTIVE / 8 / duration; profiles/mfma_shape_ab.txt).
//
//  * Operands go HBM -> LDS with global_load_lds_dwordx4 (no VGPR round trip), double buffered, one
//    barrier per K tile.  The LDS image is lane-linear, so the bank swizzle (16-byte chunk index XOR
//    ((row>>1)&7), conflict-free for the lane groups of ds_read_b128 - {0-3,12-15,20-27}, {4-11,16-19,28-31}, the same + 32 -
//    at a 128-byte row pitch: a group holds the 16 rows of a fragment, 12 of them at chunk c and 4 at c^1) is
//    applied to the per-lane SOURCE address and again on the fragment read.
//  * AMODE_CONV turns the A operand into an implicit 3x3 convolution over a zero-padded channels-last
//    image [img][S+2][S+2][Cin]: K index = (c/64, tap, c%64); every A row is a pixel whose address is shifted by
//    the tap, so no im2col buffer exists.  Rows are enumerated window-major (m = 4*window + q,
//    q = dy*2+dx inside a 2x2 pooling window) so that a 2x2 max-pool is a pure in-register max over the
//    four accumulator registers a lane holds for one window (MFMA C layout: column = lane&15, row = 4*(lane>>4) + reg).
//  * Epilogues fuse what the reference does after each contraction (bias, tanh, ReLU, dropout, 2x2
//    max-pool + argmax, one-hot label columns of fc2 as a per-object row gather, ReLU-mask for dgrad).
#pragma once
#include "common.h"
#include <type_traits>

enum { AMODE_PLAIN = 0, AMODE_CONV = 1, AMODE_CONV_GATHER = 2 };   // GATHER: conv rows come from a list of 2x2 windows (see NtParams::gather)
enum { EPI_STORE = 0, EPI_BIAS_TANH = 1, EPI_BIAS_RELU = 2, EPI_POOL = 3, EPI_FC2 = 4, EPI_RELUMASK = 5, EPI_STORE_F32 = 6,
       EPI_STORE_F32T = 7 };   // F32T (ping-pong block only): accumulators held TRANSPOSED (operands swapped in the MFMA), see nt_epilogue_f32t

struct NtParams {
    const u16* A; const u16* B; void* C;
    int M, N, K;
    long lda, ldb, ldc;
    int lgS, Cin;               // AMODE_CONV: image side S = 1<<lgS, channels per tap
    const float* bias;          // [N] or nullptr
    const u16* mask_src;        // EPI_RELUMASK: forward activation [M][ldc], gradient passes where it is > 0
    const float* lsub; const float* lobj; const int* sub_idx; const int* obj_idx;   // EPI_FC2
    unsigned char* argmax;      // EPI_POOL (optional)
    u16* C2;                    // EPI_POOL (optional): bf16 copy of the pooled output (operand of the fc1 weight gradient)
    float scale;                // EPI_RELUMASK / dropout scale
    unsigned drop_seed; int drop_enable;
    int tiles_m, tiles_n;
    int epi_lds;                // 1: LDS-staged 16-byte stores for EPI_STORE in the 8-wave kernels (set by the launcher)
    int halo_walk;              // conv16_halo_pp_kernel: 0 = block id -> (image, N tile) directly, 1 = XCD-contiguous image ranges
    int patch_aligned;          // gemm_nt_pp_kernel: 1 = grid padded to whole 32-tile patches (set by the launcher for large grids)
    const u16* Apool; const unsigned char* Acode;   // conv16_halo_pp_kernel<.., ASRC = 1>: the A operand as POOLED rows [img*64 windows][Cin]
                                                    // + routing byte (0..3 = position inside the 2x2 window, 4 = none); un-pooled on the fly
    const int* gather; const int* gather_n;         // AMODE_CONV_GATHER: row m = 4*e + q is pixel q of window gather[e] = image*(S/2)^2 + window;
                                                    // *gather_n = number of list entries (device side; p.M is only the launch bound);
                                                    // EPI_POOL writes entry e to pooled row gather[e]
                                                    // gemm_nt_pp_rows_kernel: gather [M] is the row table of A (row m = row gather[m] of A)
    // window-major row space of the shared fc1 (csrc/kernels_shared.hip): rows grouped by pooling window, groups padded to 256 rows
    const int* dest;                                // AMODE_CONV_GATHER + EPI_POOL: y / bf16 copy of entry e go to row dest[e] (argmax stays at gather[e])
    const int* wm_goff;                             // EPI_POOL: y / bf16 copy of pooled row r go to row wm_goff[r & 63] + (r >> 6) (argmax stays at r)
    float* raw; int raw_first;                      // AMODE_CONV_GATHER + EPI_POOL: the accumulators (no bias / ReLU / pooling) of the entries
                                                    // e >= raw_first also go to raw[(e - raw_first) * 4 + pixel][ldc] (linear pairs, kernels_shared.hip)
    const int* tile_group; long group_stride;       // gemm_nt_pp_kernel: M tile t multiplies with B + tile_group[t] * group_stride
    u16* Cx; int x_first;                           // nt_epilogue_f32t (fc1 over the window-major rows): rows whose index inside their group (row -
                                                    // wm_goff[tile_group[tile]]) is >= x_first - the pair-specific X rows - leave as f16 to Cx [M][N]
                                                    // instead of f32 to C; the per-object rows in front of them (2-D prefix sums follow) stay f32
    long seg_stride; int seg_bpad, seg_split;       // gemm_nt_pp_kernel<SEG>: elements between the segments (own pixels q) of a row of A; padding of B_pp's rows;
                                                    // 1 = the four centre patch pixels in two slots of two combinations
};

template <int ELEM>
__device__ __forceinline__ f32x16 mfma32(s16x8 a, s16x8 b, f32x16 c) {
    if constexpr (ELEM == ELEM_F16) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    } else {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
}

// The instruction of the NT family.  Lane l supplies row (a) / column (b) l&15 with k = 8*(l>>4) .. +7 of the 32, and holds
// column l&15, rows 4*(l>>4) + r of the 16x16 result (sgc_dbg_mfma16_probe, tests/test_mfma16_gpu.py).
template <int ELEM>
__device__ __forceinline__ f32x4 mfma16(s16x8 a, s16x8 b, f32x4 c) {
    if constexpr (ELEM == ELEM_F16) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    } else {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
}

// Row, inside a wave's output tile, of row r (0..15) of the wave's 16-row fragment i.  HALO (conv16_halo_pp_kernel): the two
// fragments of a 32-row band (the 8 windows of one window row of the map) take its even and its odd windows.
template <bool HALO>
__device__ __forceinline__ int frag_row(int i, int r) {
    if constexpr (HALO) return (i >> 1) * 32 + ((2 * (r >> 2) + (i & 1)) << 2) + (r & 3);
    else return i * 16 + r;
}

// window-major row -> element offset of padded pixel (tap 0,0) in [img][S+2][S+2][Cin]
__device__ __forceinline__ long conv_row_base(int m, int lgS, int Cin) {
    const int S = 1 << lgS;
    const int img = m >> (2 * lgS);
    const int ml = m & (S * S - 1);
    const int W = ml >> 2, q = ml & 3;
    const int py = W >> (lgS - 1), px = W & ((S >> 1) - 1);
    const int y = 2 * py + (q >> 1), x = 2 * px + (q & 1);
    return ((long)(img * (S + 2) + y) * (S + 2) + x) * Cin;
}

// FM x FN fragments of 16 x 16 per wave: fragment (i, j) holds rows frag_row(i, 4*(lane>>4) + r), column j*16 + (lane&15) of the wave's tile
template <int ELEM, int EPI, int FM, int FN, bool GATHER = false, bool HALO = false>
__device__ __forceinline__ void nt_epilogue(const NtParams& p, f32x4 (&acc)[FM][FN], int m0, int n0, int wr, int wc, int lane, int m_limit = -1) {
    const int M = GATHER ? m_limit : p.M;
    const int g = lane >> 4, cl = lane & 15;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            const int col = n0 + wc * FN * 16 + j * 16 + cl;
            const int rbase = m0 + wr * FM * 16 + frag_row<HALO>(i, 4 * g);       // the lane's four rows: one pooling window
            const float bias = p.bias ? p.bias[col] : 0.f;
            if constexpr (EPI == EPI_POOL) {
                u16* out = reinterpret_cast<u16*>(p.C);
                float v = acc[i][j][0];
                int am = 0;
#pragma unroll
                for (int q = 1; q < 4; ++q) {
                    const float t = acc[i][j][q];
                    if (t > v) { v = t; am = q; }
                }
                v += bias;
                const int prow = rbase >> 2;
                if (prow * 4 < M) {
                    long arow = prow, yrow = prow;
                    if constexpr (GATHER) {
                        arow = p.gather[prow]; yrow = p.dest ? p.dest[prow] : arow;
                        if (p.raw && prow >= p.raw_first) {
#pragma unroll
                            for (int q = 0; q < 4; ++q) p.raw[((long)(prow - p.raw_first) * 4 + q) * p.ldc + col] = acc[i][j][q];
                        }
                    }
                    else if (p.wm_goff) yrow = p.wm_goff[prow & 63] + (prow >> 6);
                    if (!(v > 0.f)) { v = 0.f; am = 4; }        // ReLU killed: no gradient path
                    out[yrow * p.ldc + col] = to_elem<ELEM>(v);
                    if (p.C2) p.C2[yrow * p.ldc + col] = f32_to_bf16_bits(v);
                    if (p.argmax) p.argmax[arow * p.ldc + col] = (unsigned char)am;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rbase + r;
                    if (row >= M) continue;
                    float v = acc[i][j][r];
                    long o = (long)row * p.ldc + col;
                    if constexpr (GATHER && EPI == EPI_STORE)      // gathered 16-bit store: back to the window-major row of the listed window
                        o = ((long)p.gather[row >> 2] * 4 + (row & 3)) * p.ldc + col;
                    if constexpr (EPI == EPI_STORE) {
                        reinterpret_cast<u16*>(p.C)[o] = to_elem<ELEM>(v + bias);
                    } else if constexpr (EPI == EPI_STORE_F32) {
                        reinterpret_cast<float*>(p.C)[o] = v + bias;
                    } else if constexpr (EPI == EPI_BIAS_TANH) {
                        reinterpret_cast<u16*>(p.C)[o] = to_elem<ELEM>(tanhf(v + bias));
                    } else if constexpr (EPI == EPI_BIAS_RELU) {
                        v = fmaxf(v + bias, 0.f);
                        if (p.drop_enable) v = dropout_keep(p.drop_seed, (uint32_t)(row * p.N + col)) ? v * p.scale : 0.f;
                        reinterpret_cast<u16*>(p.C)[o] = to_elem<ELEM>(v);
                    } else if constexpr (EPI == EPI_FC2) {
                        v += bias + p.lsub[(long)p.sub_idx[row] * p.N + col] + p.lobj[(long)p.obj_idx[row] * p.N + col];
                        v = fmaxf(v, 0.f);
                        if (p.drop_enable) v = dropout_keep(p.drop_seed, (uint32_t)(row * p.N + col)) ? v * p.scale : 0.f;
                        reinterpret_cast<float*>(p.C)[o] = v;
                    } else if constexpr (EPI == EPI_RELUMASK) {
                        const float f = from_elem<ELEM_F16>(p.mask_src[o]);   // forward activations are f16
                        reinterpret_cast<u16*>(p.C)[o] = to_elem<ELEM>(f > 0.f ? v * p.scale : 0.f);
                    }
                }
            }
        }
    }
}

// f32 output of the 8-wave 256x256 block with the operands SWAPPED in the MFMA (acc = B_frag x A_frag^T): a lane then owns one output
// ROW (m = lane & 15) and the four consecutive COLUMNS 4*(lane>>4) .. +3 of every fragment, so the tile leaves as 32 16-byte stores per
// lane instead of the 128 4-byte stores of the plain C layout (fc1 over window-major rows: 5 GB of f32 products per launch, K = 1024 -
// the epilogue is as long as the main loop).  Same products, same order of accumulation over k: bit-identical to EPI_STORE_F32.
__device__ __forceinline__ void nt_epilogue_f32t(const NtParams& p, f32x4 (&acc)[8][4], int m0, int n0, int wr, int wc, int lane) {
    const int g = lane >> 4, cl = lane & 15;
    float* out = reinterpret_cast<float*>(p.C);
    if (!out) return;                                  // no output buffer: the launch without its stores
    const int g_first = p.Cx ? p.wm_goff[p.tile_group[m0 >> 8]] + p.x_first : 0;      // first X row of this tile's group
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int row = m0 + wr * 128 + i * 16 + cl;
        if (row >= p.M) continue;
        const bool xrow = p.Cx && row >= g_first;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + wc * 64 + j * 16 + 4 * g;
            f32x4 v = acc[i][j];
            if (p.bias) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(p.bias + col);
                v += b;
            }
            if (xrow) {                                // a pair-specific row: one of ~7 products added per pair, f16 carries it
                uint2 hv;
                hv.x = (unsigned)f32_to_f16_bits(v[0]) | ((unsigned)f32_to_f16_bits(v[1]) << 16);
                hv.y = (unsigned)f32_to_f16_bits(v[2]) | ((unsigned)f32_to_f16_bits(v[3]) << 16);
                *reinterpret_cast<uint2*>(p.Cx + (long)row * p.N + col) = hv;
                continue;
            }
            f32x4* dst = reinterpret_cast<f32x4*>(out + (long)row * p.ldc + col);
            *dst = v;
        }
    }
}

// Tile walk order: the tiles_m x tiles_n grid is traversed in 16 x 16 super-tiles (N fastest inside a super-tile), so
// the ~256 blocks in flight cover a square patch of the output: each A row-panel is shared by 16 blocks and each B
// row-panel by 16 blocks through L2 / Infinity Cache.  With the plain "N fastest" order a GEMM with many N tiles
// (fc1 data gradient: 126 x 256 tiles) re-streams the whole B operand from HBM for every M tile (63 GB per launch).
__device__ __forceinline__ void supertile_map(int id, int tiles_m, int tiles_n, int& tm, int& tn) {
    constexpr int GS = 16;
    const int a = id / (GS * tiles_n);
    const int hm = min(GS, tiles_m - a * GS);
    const int id2 = id - a * GS * tiles_n;
    const int sn = (tiles_n + GS - 1) / GS;
    const int b = min(id2 / (hm * GS), sn - 1);
    const int id3 = id2 - b * hm * GS;
    const int wn = min(GS, tiles_n - b * GS);
    tm = a * GS + id3 / wn;
    tn = b * GS + id3 % wn;
}

__device__ __forceinline__ void supertile_map_g(int id, int tiles_m, int tiles_n, int GM, int GN, int& tm, int& tn) {
    const int a = id / (GM * tiles_n);
    const int hm = min(GM, tiles_m - a * GM);
    const int id2 = id - a * GM * tiles_n;
    const int sn = (tiles_n + GN - 1) / GN;
    const int b = min(id2 / (hm * GN), sn - 1);
    const int id3 = id2 - b * hm * GN;
    const int wn = min(GN, tiles_n - b * GN);
    tm = a * GM + id3 / wn;
    tn = b * GN + id3 % wn;
}

// LDS-staged epilogue for 16-bit EPI_STORE outputs of the 8-wave 256x256 block (conv3 / fc1 / conv2 data gradients write
// 4-9 GB per launch): the MFMA C layout gives each lane ONE column (four rows per fragment), i.e. 2-byte global stores.  Here
// each wave transposes its 128x64 sub-tile through its own 18 KiB LDS region (row pitch 144 B): neighbouring lanes swap a
// value (DPP) so that every lane writes one packed dword (two adjacent columns), then the wave reads rows back as 16-byte
// pieces and issues 16 full-line 16-byte stores per lane instead of 128 2-byte ones.  Needs 8 x 16 KiB of LDS.
// Row pitch 128 B (no padding): the read-back is a ds_read_b128 whose 16-lane groups cover rows (r, r+1, r+2, r+3) x half a row -
// with 32 dwords per row the four pieces land on disjoint quarters of the 64 banks; the dword writes of an (even, odd) lane pair
// would fall on one bank two-way (free for a ds_write_b32, but counted): odd rows swap their halves.  Rounds 2-4 padded the rows to 144 B:
// conflict-light writes, but two-way conflicts on every read (SQ_LDS_BANK_CONFLICT 5.6 % of the LDS-active cycles of the window
// data gradient, 2.8 % of fc1's).
constexpr int EPI_LDS_PITCH = 128;
constexpr int EPI_LDS_BYTES = 8 * 128 * EPI_LDS_PITCH;
// MASK (EPI_RELUMASK through this epilogue, round 5): the value is multiplied by p.scale before it is rounded, and the read-back zeroes the
// elements whose forward activation p.mask_src (f16, the output's shape) is not > 0 - 16-byte mask loads beside the 16-byte stores; the
// generic epilogue did this with a 2-byte load and a 2-byte store per element (fc2's data gradient: 0.50 ms for 0.5 GB).  Same values.
// On the 16x16 fragments a lane holds rows 4*(lane>>4) + r of one column: the (even, odd) lane pair swaps, every lane writes the packed dword of one row.
// (The sparse data gradient keeps 32-row accumulators and its own copy of this epilogue, csrc/kernels_dgrad_sp.hip.)
// The rows 4g of the four lane groups are all even: besides the half swap of odd rows, rows with bit 2 set swap their 32-byte quarters, so the
// 32 lanes of a ds_write_b32 pass (g = 0,1 or 2,3; 8 dwords each for even and odd rows) cover 32 distinct banks; the read-back applies both.
template <int ELEM, bool MASK = false, bool HALO = false>
__device__ __forceinline__ void nt_epilogue_store16(const NtParams& p, f32x4 (&acc)[8][4], int m0, int n0, int wr, int wc, int lane,
                                                    int wid, char* smem) {
    __syncthreads();                                   // every wave is done reading operand tiles
    char* reg = smem + wid * (128 * EPI_LDS_PITCH);
    const int g = lane >> 4, cl = lane & 15;
    const bool odd = cl & 1;
    constexpr int QB = HALO ? 8 : 4;                   // the row bit that lane>>4 & 1 lands on (frag_row)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + wc * 64 + j * 16 + cl;
            const float bias = p.bias ? p.bias[col] : 0.f;
#pragma unroll
            for (int rp = 0; rp < 2; ++rp) {
                float v0 = acc[i][j][2 * rp] + bias, v1 = acc[i][j][2 * rp + 1] + bias;
                if constexpr (MASK) { v0 *= p.scale; v1 *= p.scale; }
                const float recv = __shfl_xor(odd ? v0 : v1, 1);
                const float flo = odd ? recv : v0, fhi = odd ? v1 : recv;
                unsigned packed;
                if constexpr (ELEM == ELEM_BF16) packed = f32x2_to_bf16x2_bits(flo, fhi);      // one v_cvt_pk_bf16_f32
                else packed = (unsigned)to_elem<ELEM>(flo) | ((unsigned)to_elem<ELEM>(fhi) << 16);
                const int row = frag_row<HALO>(i, 4 * g + 2 * rp) + (odd ? 1 : 0);
                *reinterpret_cast<unsigned*>(reg + row * EPI_LDS_PITCH + (((j * 16 + (cl & ~1)) * 2) ^ ((row & 1) << 6) ^ ((row & QB) ? 32 : 0))) = packed;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    u16* out = reinterpret_cast<u16*>(p.C);
    const int c8 = lane & 7, rsub = lane >> 3;
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int rowl = it * 8 + rsub;
        uint4 v = *reinterpret_cast<const uint4*>(reg + rowl * EPI_LDS_PITCH + ((c8 * 16) ^ ((rowl & 1) << 6) ^ ((rowl & QB) ? 32 : 0)));
        const int row = m0 + wr * 128 + rowl;
        if (row < p.M) {
            const long o = (long)row * p.ldc + n0 + wc * 64 + c8 * 8;
            if constexpr (MASK) {
                const uint4 f = *reinterpret_cast<const uint4*>(p.mask_src + o);
                const u16* fh = reinterpret_cast<const u16*>(&f);
                u16* vh = reinterpret_cast<u16*>(&v);
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (!(from_elem<ELEM_F16>(fh[k]) > 0.f)) vh[k] = 0;
            }
            *reinterpret_cast<uint4*>(out + o) = v;
        }
    }
}

// Block configuration: WR x WC wavefronts, each owning a (TM*32) x (TN*32) output tile = FM x FN = 2TM x 2TN fragments of 16 x 16.
//   small: 2x2 waves of 64x64   -> 128x128 block, 64 KiB LDS, 2 blocks/CU  (small problems, N % 256 != 0)
//   big  : 2x4 waves of 128x64  -> 256x256 block, 128 KiB LDS, 1 block/CU  (half the LDS bytes per MFMA)
template <int ELEM, int AMODE, int EPI, int WR, int WC, int TM, int TN>
__global__ __launch_bounds__(WR * WC * 64, 2) void gemm_nt_kernel(const NtParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NW = WR * WC;
    constexpr int BM = WR * TM * 32, BN = WC * TN * 32;
    constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, BUF_BYTES = A_BYTES + B_BYTES;
    constexpr int AI = BM / (8 * NW), BI = BN / (8 * NW);      // global_load_lds instructions per wave per K tile
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    int tm, tn;
    supertile_map(blockIdx.x, p.tiles_m, p.tiles_n, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    int Mlim = p.M;
    if constexpr (AMODE == AMODE_CONV_GATHER) {
        Mlim = min(p.M, 4 * *p.gather_n);
        if (m0 >= Mlim) return;                     // the grid is sized for the bound, the list is usually shorter
    }

    // ---- loader addresses: wave w stages rows w*AI*8 .. of A and w*BI*8 .. of B, 8 rows (1 KiB) per instruction
    const int lrow = lane >> 3, cpos = lane & 7;
    const u16* a_ptr[AI];
    const u16* b_ptr[BI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        const int row = wid * AI * 8 + i * 8 + lrow;
        const int chunk = cpos ^ ((row >> 1) & 7);
        int m = m0 + row; if (m > Mlim - 1) m = Mlim - 1;
        if constexpr (AMODE == AMODE_CONV_GATHER) m = p.gather[m >> 2] * 4 + (m & 3);
        if constexpr (AMODE != AMODE_PLAIN) a_ptr[i] = p.A + conv_row_base(m, p.lgS, p.Cin) + chunk * 8;
        else a_ptr[i] = p.A + (long)m * p.lda + chunk * 8;
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
        const int row = wid * BI * 8 + i * 8 + lrow;
        const int chunk = cpos ^ ((row >> 1) & 7);
        b_ptr[i] = p.B + (long)(n0 + row) * p.ldb + chunk * 8;
    }
    const int Wp = (1 << p.lgS) + 2;

    auto stage = [&](int buf, int kt) {
        long aoff;
        if constexpr (AMODE != AMODE_PLAIN) {
            // K order = (64-channel chunk, tap, channel): the nine taps of one chunk are consecutive K tiles, so
            // the shifted re-reads of a pixel row hit L2 (working set 18x18x64 ch per block) instead of the fabric.
            const int cc = kt / 9, tap = kt - cc * 9;
            const int ky = tap / 3, kx = tap - 3 * ky;
            aoff = (long)(ky * Wp + kx) * p.Cin + (cc << 6);
        } else {
            aoff = (long)kt << 6;
        }
        const long boff = (long)kt << 6;
        char* abase = smem + buf * BUF_BYTES + wid * (AI * 1024);
        char* bbase = smem + buf * BUF_BYTES + A_BYTES + wid * (BI * 1024);
#pragma unroll
        for (int i = 0; i < AI; ++i)
            __builtin_amdgcn_global_load_lds(GLB_PTR(a_ptr[i] + aoff), LDS_PTR(abase + i * 1024), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < BI; ++i)
            __builtin_amdgcn_global_load_lds(GLB_PTR(b_ptr[i] + boff), LDS_PTR(bbase + i * 1024), 16, 0, 0);
    };

    // ---- fragment read addresses
    const int wr = wid / WC, wc = wid % WC;
    // fragment i of a wave = 16 rows; the row swizzle (row>>1)&7 only depends on lane&15 (fragments start at multiples of 16 rows)
    const int kg = lane >> 4, sw = ((lane & 15) >> 1) & 7;
    constexpr int FM = 2 * TM, FN = 2 * TN;
    const int a_rd = (wr * TM * 32 + (lane & 15)) * 128, b_rd = (wc * TN * 32 + (lane & 15)) * 128;
    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

    const int nk = p.K >> 6;
    stage(0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
        const char* ab = smem + (kt & 1) * BUF_BYTES;
        const char* bb = ab + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {               // one instruction step = 32 k = chunks 4*ks .. +3, one per lane group
            const int ko = ((ks * 4 + kg) ^ sw) << 4;
            s16x8 af[FM], bf[FN];
#pragma unroll
            for (int i = 0; i < FM; ++i) af[i] = *reinterpret_cast<const s16x8*>(ab + a_rd + i * 2048 + ko);
#pragma unroll
            for (int i = 0; i < FN; ++i) bf[i] = *reinterpret_cast<const s16x8*>(bb + b_rd + i * 2048 + ko);
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j) acc[i][j] = mfma16<ELEM>(af[i], bf[j], acc[i][j]);
        }
    }

    if constexpr (EPI == EPI_STORE && TM == 4 && TN == 2 && WR * WC == 8) {
        if (p.epi_lds) { nt_epilogue_store16<ELEM>(p, acc, m0, n0, wr, wc, lane, wid, smem); return; }
    }
    if constexpr (AMODE == AMODE_CONV_GATHER) nt_epilogue<ELEM, EPI, FM, FN, true>(p, acc, m0, n0, wr, wc, lane, Mlim);
    else nt_epilogue<ELEM, EPI, FM, FN>(p, acc, m0, n0, wr, wc, lane);
}

template <int ELEM, int AMODE, int EPI, int WR, int WC, int TM, int TN>
static int launch_gemm_nt_cfg(NtParams p, hipStream_t stream) {
    constexpr int BM = WR * TM * 32, BN = WC * TN * 32;
    constexpr int LDS0 = 2 * (BM + BN) * 128;
    constexpr int LDS = (EPI == EPI_STORE && TM == 4 && TN == 2 && WR * WC == 8 && LDS0 < EPI_LDS_BYTES) ? EPI_LDS_BYTES : LDS0;
    p.tiles_m = (p.M + BM - 1) / BM;
    p.tiles_n = p.N / BN;
    auto kern = gemm_nt_kernel<ELEM, AMODE, EPI, WR, WC, TM, TN>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    SGC_LAUNCH(kern, dim3((unsigned)(p.tiles_m * p.tiles_n)), dim3(WR * WC * 64), LDS, stream, p);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}


#include "gemm_nt_pp.h"

// One schedule per shape and mode.  Outputs of M x N >= 256^3 elements with N % 256 == 0 take a 256x256 block: the halo-staged
// ping-pong block for 3x3 convolutions on 16x16 maps, the ping-pong block for plain rows, the 2-stage block for the other
// convolutions (conv2's 32x32 maps).  Everything else takes the 128x128 block.
template <int ELEM, int AMODE, int EPI>
static int launch_gemm_nt(NtParams p, hipStream_t stream) {
    static_assert(AMODE == AMODE_PLAIN || AMODE == AMODE_CONV, "gathered rows have their own launchers");
    if (p.M <= 0) return SGC_OK;
    if ((p.K & 63) || (p.N & 127) || p.K <= 0) return SGC_ERR_ARG;
    if (AMODE == AMODE_CONV && ((p.Cin & 63) || p.K != 9 * p.Cin)) return SGC_ERR_ARG;
    p.epi_lds = 1;                         // 16-bit outputs of the 256x256 blocks leave through LDS as 16-byte stores
    const bool big = (p.N % 256) == 0 && (long)p.M * p.N >= 256L * 256 * 256;
    if constexpr (AMODE == AMODE_CONV && (EPI == EPI_POOL || EPI == EPI_STORE)) {
        if (big && p.lgS == 4 && (p.M % 256) == 0) return launch_conv16_halo_pp<ELEM, EPI>(p, stream);
    }
    if (big) {
        if constexpr (AMODE == AMODE_PLAIN) return launch_gemm_nt_pp<ELEM, EPI>(p, stream);
        else return launch_gemm_nt_cfg<ELEM, AMODE, EPI, 2, 4, 4, 2>(p, stream);
    }
    return launch_gemm_nt_cfg<ELEM, AMODE, EPI, 2, 2, 2, 2>(p, stream);
}
