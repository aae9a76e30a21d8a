// Input gradient of conv1 (reference model.py:139-140, the 1x1 convolutions conv1_1 / conv1_2 on train_test.py:194-195's
// cat(image_feature, image_depth)): the gradient that leaves the relation head towards whatever produced its inputs.
//
//   dX[img][c][pix] = sum_r sum_k dpre1_r[img*HW + pix][k] * W1_r[k][c]          c = 0..256, k = 0..127, r = role (subject / object)
//
// conv1 runs once per image and role, so this is one small product per step ([n_img*1024] x 257 x 256: 8192 x 257 x 256 at 8 images,
// ~13 MB moved) - launch- and memory-bound.  One launch, no split-K, no atomics: every output element has one owner that sums role a's
// K then role b's K in a fixed order, so two runs give identical bits.
//
// v_mfma_f32_32x32x16_bf16 with W1^T as the A operand (row = channel) and dpre1 as the B operand (column = pixel): a lane's fragments
// are 16 contiguous bytes of a W1^T row / a dpre1 row, read where they lie (the 74 KB per role of W1^T stay in L2), and the accumulator
// has the pixel on the lane - one register of it is 32 consecutive f32 of one NCHW channel row (two 128-byte segments per store
// instruction), so the NCHW f32 output needs no transpose.  A wave owns one [32 channels] x [32 pixels] tile: 16 MFMAs with both roles.
// Rows of the padded channels (257 .. CP-1, zero in W1^T) are never stored.
#include "common.h"

namespace {

constexpr int DG_K = 128;        // conv1 output channels per role = the K of one role

__global__ __launch_bounds__(256) void conv1_dgrad_kernel(const u16* __restrict__ dpre_a, const u16* __restrict__ wt_a,
                                                          const u16* __restrict__ dpre_b, const u16* __restrict__ wt_b,
                                                          float* __restrict__ out0, int C0, float* __restrict__ out1, int C1,
                                                          long n_pix, int HW, int accumulate) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long pix0 = ((long)blockIdx.x * 4 + wave) * 32;
    if (pix0 >= n_pix) return;                                   // n_pix is a multiple of 32 (HW is): whole tiles only
    const int r = lane & 31, h = lane >> 5;
    const int c0 = blockIdx.y * 32;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int role = 0; role < 2; ++role) {
        const u16* dp = role ? dpre_b : dpre_a;
        const u16* wt = role ? wt_b : wt_a;
        if (dp == nullptr) continue;                             // uniform over the grid
        const u16* ap = wt + (long)(c0 + r) * DG_K + 8 * h;      // A[row = channel c0 + r][k = 16 s + 8 h + j]
        const u16* bp = dp + (pix0 + r) * DG_K + 8 * h;          // B[k = 16 s + 8 h + j][col = pixel pix0 + r]
#pragma unroll
        for (int s = 0; s < DG_K / 16; ++s) {
            const s16x8 a = *reinterpret_cast<const s16x8*>(ap + 16 * s);
            const s16x8 b = *reinterpret_cast<const s16x8*>(bp + 16 * s);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
        }
    }
    const long pix = pix0 + r;
    const long img = pix / HW;
    const long p = pix - img * HW;
    const int C = C0 + C1;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = c0 + (i & 3) + 8 * (i >> 2) + 4 * h;      // accumulator register i of lane half h
        if (c >= C) continue;                                    // padded channel rows: never stored
        float* dst = c < C0 ? out0 + (img * C0 + c) * HW + p : out1 + (img * C1 + (c - C0)) * HW + p;
        *dst = accumulate ? *dst + acc[i] : acc[i];
    }
}

}  // namespace

extern "C" {

int sgc_conv1_dgrad(const void* dpre_a, const void* wt_a, const void* dpre_b, const void* wt_b, float* out0, int C0, float* out1, int C1,
                    int n_img, int HW, int accumulate, void* stream) {
    if ((dpre_a == nullptr) != (wt_a == nullptr) || (dpre_b == nullptr) != (wt_b == nullptr)) return SGC_ERR_ARG;
    if (dpre_a == nullptr && dpre_b == nullptr) return SGC_ERR_ARG;
    if (out0 == nullptr || C0 <= 0 || C1 < 0 || (out1 == nullptr) != (C1 == 0) || C0 + C1 != 257) return SGC_ERR_ARG;
    if (n_img < 0 || HW <= 0 || (HW & 31)) return SGC_ERR_ARG;
    if ((((uintptr_t)dpre_a | (uintptr_t)wt_a | (uintptr_t)dpre_b | (uintptr_t)wt_b) & 15) != 0) return SGC_ERR_ARG;      // 16-byte fragments
    if (n_img == 0) return SGC_OK;
    const long n_pix = (long)n_img * HW;
    const int CP = (C0 + C1 + 31) / 32 * 32;
    SGC_LAUNCH(conv1_dgrad_kernel, dim3((unsigned)((n_pix / 32 + 3) / 4), CP / 32), dim3(256), 0, (hipStream_t)stream, (const u16*)dpre_a,
               (const u16*)wt_a, (const u16*)dpre_b, (const u16*)wt_b, out0, C0, out1, C1, n_pix, HW, accumulate);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

}  // extern "C"
