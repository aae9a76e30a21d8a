// Fused multi-head attention forward for head dim 32 (the 18 attention blocks of the DETR-101 extractor, detr.py): flash-style,
// online softmax over key tiles, key-padding mask, no [L, L] matrix in HBM.
//
// One workgroup = 4 wavefronts = 64 query rows of one (image, head); a wavefront owns 16 query rows.  Keys are walked in tiles of
// 64: the K tile [key][d] and the transposed V tile [d][key] are staged through LDS (the next tile's global loads are in flight
// while the current one is consumed), the tile's mask bytes next to them.
//
// Orientation (MFMA maps: gemm_nt.h mfma16, tests/test_mfma16_gpu.py; the f32 16x16x4 form has A[l&15][k=l>>4], B[k=l>>4][l&15] and the
// same C/D map): both products are computed transposed so that a lane owns ONE query, c = lane&15, in every register it holds.
//   S^T = K Q^T : A = K tile rows, B = Q.  Register r of key subtile t is the score of key 16t + 4g + r (g = lane>>4) for query c.
//                 16-bit: head dim 32 is the whole K of one v_mfma_f32_16x16x32; f32: 8 x v_mfma_f32_16x16x4_f32 (exact f32 chain).
//   O^T = V^T P^T : A = V^T (row = d), B = P^T.  The lane's own P registers ARE the B operand: k slot 8g + j of a 32-key step stands for
//                 key 32s + 16(j>>2) + 4g + (j&3), and the V^T fragment is read from LDS in that same order (two 8-byte reads).
// So the running max, the running sum and the rescale factor are per-lane scalars; the only cross-lane traffic of the softmax is the
// reduction over the four lanes l, l^16, l^32, l^48 that share a query.  Softmax, max and sum are f32; P is rounded to the input type
// only as the PV operand, the row sum adds the unrounded P.  No atomics, one summation order: two runs give the same bits.
#include "common.h"
#include "sgc_relhead.h"
#include <math.h>

namespace {

constexpr int ATT_D = 32;        // head dim
constexpr int ATT_QB = 64;       // query rows per workgroup (16 per wavefront)
constexpr int ATT_KT = 64;       // keys per tile

enum { ATT_F32 = 0, ATT_F16 = 1, ATT_BF16 = 2 };

template <int DT> struct AttT;
template <> struct AttT<ATT_F32> { typedef float elem; static constexpr int KLD = 36, VLD = 68; };
template <> struct AttT<ATT_F16> { typedef u16 elem; static constexpr int KLD = 40, VLD = 72; };
template <> struct AttT<ATT_BF16> { typedef u16 elem; static constexpr int KLD = 40, VLD = 72; };

template <int DT> __device__ __forceinline__ u16 att_round(float f) {
    if constexpr (DT == ATT_F16) return f32_to_f16_bits(f); else return f32_to_bf16_bits(f);
}

template <int DT>
__global__ __launch_bounds__(256) void mha_fwd_kernel(const void* __restrict__ qv, const void* __restrict__ kv, const void* __restrict__ vv,
                                                      const unsigned char* __restrict__ kpm, void* __restrict__ ov, int Lq, int Lk, int H,
                                                      int nqb, long q_sL, long q_sB, long k_sL, long k_sB, long v_sL, long v_sB, long o_sL,
                                                      long o_sB, float scale) {
    typedef typename AttT<DT>::elem E;
    constexpr int KLD = AttT<DT>::KLD, VLD = AttT<DT>::VLD;
    constexpr int CH = 16 / (int)sizeof(E);             // elements per 16-byte chunk
    constexpr int CPR = ATT_D / CH;                     // chunks per row
    constexpr int NCH = ATT_KT * CPR / 256;             // chunks per thread and tile (f32: 2, 16-bit: 1)
    __shared__ __attribute__((aligned(16))) E Ks[ATT_KT * KLD];
    __shared__ __attribute__((aligned(16))) E Vt[ATT_D * VLD];
    __shared__ __attribute__((aligned(16))) unsigned char Ms[ATT_KT];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int qb = blockIdx.x % nqb, bh = blockIdx.x / nqb;
    const int b = bh / H, h = bh % H;
    const E* q = (const E*)qv + (long)b * q_sB + h * ATT_D;
    const E* k = (const E*)kv + (long)b * k_sB + h * ATT_D;
    const E* v = (const E*)vv + (long)b * v_sB + h * ATT_D;
    E* o = (E*)ov + (long)b * o_sB + h * ATT_D;
    const unsigned char* mrow = kpm ? kpm + (long)b * Lk : nullptr;

    // this lane's query row, d = 8g .. 8g+7 (rows past Lq compute on zeros and are not stored)
    const int qi = qb * ATT_QB + wave * 16 + c;
    uint4 qraw[CH == 4 ? 2 : 1];
#pragma unroll
    for (int i = 0; i < (CH == 4 ? 2 : 1); ++i) {
        qraw[i] = make_uint4(0, 0, 0, 0);
        if (qi < Lq) qraw[i] = *(const uint4*)(q + (long)qi * q_sL + 8 * g + i * CH);
    }

    uint4 kreg[NCH], vreg[NCH];
    unsigned char mreg = 1;
    auto load_tile = [&](int j0) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int ch = tid + i * 256, row = ch / CPR, col = (ch % CPR) * CH;
            kreg[i] = make_uint4(0, 0, 0, 0);
            vreg[i] = make_uint4(0, 0, 0, 0);
            if (j0 + row < Lk) {
                kreg[i] = *(const uint4*)(k + (long)(j0 + row) * k_sL + col);
                vreg[i] = *(const uint4*)(v + (long)(j0 + row) * v_sL + col);
            }
        }
        if (tid < ATT_KT) {
            const int j = j0 + tid;
            mreg = 1;                                    // keys past Lk are masked keys
            if (j < Lk) mreg = mrow ? (mrow[j] != 0) : 0;
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int ch = tid + i * 256, row = ch / CPR, col = (ch % CPR) * CH;
            *(uint4*)(Ks + row * KLD + col) = kreg[i];
            E tmp[CH];
            *(uint4*)tmp = vreg[i];
#pragma unroll
            for (int e = 0; e < CH; ++e) Vt[(col + e) * VLD + row] = tmp[e];
        }
        if (tid < ATT_KT) Ms[tid] = mreg;
    };

    float m = -INFINITY, l = 0.f;                        // running max of the query; this LANE's part of the running sum
    f32x4 oacc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};     // O^T[d = 16*db + 4g + r][query c]

    const int nt = (Lk + ATT_KT - 1) / ATT_KT;
    if (nt > 0) load_tile(0);
    for (int t = 0; t < nt; ++t) {
        __syncthreads();                                 // every wavefront is done reading the previous tile
        store_tile();
        __syncthreads();
        if (t + 1 < nt) load_tile((t + 1) * ATT_KT);     // in flight during the products below

        // ---- scores S^T = K Q^T
        f32x4 sc[4];
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const E* kp = Ks + (t4 * 16 + c) * KLD + 8 * g;
            if constexpr (DT == ATT_F32) {
                float kf[8], qf[8];
                *(uint4*)kf = *(const uint4*)kp;
                *(uint4*)(kf + 4) = *(const uint4*)(kp + 4);
                *(uint4*)qf = qraw[0];
                *(uint4*)(qf + 4) = qraw[1];
#pragma unroll
                for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s], qf[s], acc, 0, 0, 0);
            } else {
                const s16x8 kf = __builtin_bit_cast(s16x8, *(const uint4*)kp);
                const s16x8 qf = __builtin_bit_cast(s16x8, qraw[0]);
                if constexpr (DT == ATT_F16)
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, kf), __builtin_bit_cast(f16x8, qf), acc, 0, 0, 0);
                else
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kf), __builtin_bit_cast(bf16x8, qf), acc, 0, 0, 0);
            }
            const uint32_t mw = *(const uint32_t*)(Ms + t4 * 16 + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) sc[t4][r] = ((mw >> (8 * r)) & 0xffu) ? -INFINITY : acc[r] * scale;
        }

        // ---- online softmax: all 16 registers belong to query c; the query's other keys sit in lanes l^16, l^32, l^48
        float mt = sc[0][0];
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4)
#pragma unroll
            for (int r = 0; r < 4; ++r) mt = fmaxf(mt, sc[t4][r]);
        mt = fmaxf(mt, __shfl_xor(mt, 16));
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float mn = fmaxf(m, mt);
        const float mu = (mn == -INFINITY) ? 0.f : mn;   // every key so far masked: exp(-inf - 0) = 0, never exp(-inf + inf)
        float alpha, ps = 0.f;
        if constexpr (DT == ATT_F32) alpha = expf(m - mu); else alpha = __expf(m - mu);
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float p;
                if constexpr (DT == ATT_F32) p = expf(sc[t4][r] - mu); else p = __expf(sc[t4][r] - mu);
                sc[t4][r] = p;
                ps += p;
            }
        m = mn;
        l = l * alpha + ps;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int r = 0; r < 4; ++r) oacc[db][r] *= alpha;

        // ---- O^T += V^T P^T
        if constexpr (DT == ATT_F32) {
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int t4 = 0; t4 < 4; ++t4) {
                    float vf[4];
                    *(uint4*)vf = *(const uint4*)(Vt + (db * 16 + c) * VLD + t4 * 16 + 4 * g);
#pragma unroll
                    for (int r = 0; r < 4; ++r) oacc[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[r], sc[t4][r], oacc[db], 0, 0, 0);
                }
        } else {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                s16x8 pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[j] = (short)att_round<DT>(sc[2 * ks + (j >> 2)][j & 3]);
#pragma unroll
                for (int db = 0; db < 2; ++db) {
                    const E* vp = Vt + (db * 16 + c) * VLD + 32 * ks + 4 * g;
                    uint2 lo = *(const uint2*)vp, hi = *(const uint2*)(vp + 16);
                    const s16x8 vf = __builtin_bit_cast(s16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
                    if constexpr (DT == ATT_F16)
                        oacc[db] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, vf), __builtin_bit_cast(f16x8, pf), oacc[db], 0, 0, 0);
                    else
                        oacc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vf), __builtin_bit_cast(bf16x8, pf), oacc[db], 0, 0, 0);
                }
            }
        }
    }

    // ---- out = O / l; a query without an unmasked key (l = 0, Lk = 0 included) gets zeros
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    const float inv = l > 0.f ? 1.f / l : 0.f;
    if (qi < Lq) {
#pragma unroll
        for (int db = 0; db < 2; ++db) {
            E* op = o + (long)qi * o_sL + db * 16 + 4 * g;
            if constexpr (DT == ATT_F32) {
                const f32x4 r = {oacc[db][0] * inv, oacc[db][1] * inv, oacc[db][2] * inv, oacc[db][3] * inv};
                *(f32x4*)op = r;
            } else {
                const uint32_t w0 = (uint32_t)att_round<DT>(oacc[db][0] * inv) | ((uint32_t)att_round<DT>(oacc[db][1] * inv) << 16);
                const uint32_t w1 = (uint32_t)att_round<DT>(oacc[db][2] * inv) | ((uint32_t)att_round<DT>(oacc[db][3] * inv) << 16);
                *(uint2*)op = make_uint2(w0, w1);
            }
        }
    }
}

// Largest element index + 1 of an [L, B, 32 H] tensor with the given strides; -1 for a stride the contract excludes.
long att_extent(int L, int B, int H, long sL, long sB, int mult) {
    if (sL < 0 || sB < 0 || sL % mult != 0 || sB % mult != 0) return -1;
    if (L == 0 || B == 0) return 0;
    const long lim = 1L << 31;
    if (sL > lim || sB > lim) return lim + 1;
    return (long)(L - 1) * sL + (long)(B - 1) * sB + (long)ATT_D * H;
}

}  // namespace

extern "C" int sgc_mha_fwd(const void* q, const void* k, const void* v, const unsigned char* key_padding_mask, void* out, int Lq, int Lk,
                           int B, int H, long q_sL, long q_sB, long k_sL, long k_sB, long v_sL, long v_sB, long o_sL, long o_sB, int dtype,
                           float scale, void* stream) {
    if (H < 1 || Lq < 0 || Lk < 0 || B < 0 || dtype < 0 || dtype > 2 || !isfinite(scale)) return SGC_ERR_ARG;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) return SGC_ERR_ARG;
    const int mult = dtype == ATT_F32 ? 4 : 8;
    const long lim = 1L << 31;
    const long eq = att_extent(Lq, B, H, q_sL, q_sB, mult), ek = att_extent(Lk, B, H, k_sL, k_sB, mult);
    const long ev = att_extent(Lk, B, H, v_sL, v_sB, mult), eo = att_extent(Lq, B, H, o_sL, o_sB, mult);
    if (eq < 0 || ek < 0 || ev < 0 || eo < 0 || eq > lim || ek > lim || ev > lim || eo > lim) return SGC_ERR_ARG;
    if ((long)B * Lk > lim) return SGC_ERR_ARG;
    if (Lq == 0 || B == 0) return SGC_OK;
    if (!q || !out || (Lk > 0 && (!k || !v))) return SGC_ERR_ARG;
    const int nqb = (Lq + ATT_QB - 1) / ATT_QB;
    const long nblk = (long)nqb * B * H;
    if (nblk >= lim) return SGC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)nblk), block(256);
    if (dtype == ATT_F32)
        SGC_LAUNCH(mha_fwd_kernel<ATT_F32>, grid, block, 0, s, q, k, v, key_padding_mask, out, Lq, Lk, H, nqb, q_sL, q_sB, k_sL, k_sB, v_sL,
                   v_sB, o_sL, o_sB, scale);
    else if (dtype == ATT_F16)
        SGC_LAUNCH(mha_fwd_kernel<ATT_F16>, grid, block, 0, s, q, k, v, key_padding_mask, out, Lq, Lk, H, nqb, q_sL, q_sB, k_sL, k_sB, v_sL,
                   v_sB, o_sL, o_sB, scale);
    else
        SGC_LAUNCH(mha_fwd_kernel<ATT_BF16>, grid, block, 0, s, q, k, v, key_padding_mask, out, Lq, Lk, H, nqb, q_sL, q_sB, k_sL, k_sB, v_sL,
                   v_sB, o_sL, o_sB, scale);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}
