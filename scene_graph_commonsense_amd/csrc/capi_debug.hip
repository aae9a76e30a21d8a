// Test hooks: raw access to the two GEMM engines (tests/test_gemm_gpu.py) and a few instruction probes.
#include "gemm_nt.h"
#include "gemm_tn.h"

extern "C" {

int sgc_dbg_gemm_nt(int elem, const void* A, const void* B, void* C, int M, int N, int K,
                    long lda, long ldb, long ldc, const float* bias, void* stream) {
    NtParams p{};
    p.A = (const u16*)A; p.B = (const u16*)B; p.C = C; p.M = M; p.N = N; p.K = K;
    p.lda = lda; p.ldb = ldb; p.ldc = ldc; p.bias = bias;
    if (elem == ELEM_F16) return launch_gemm_nt<ELEM_F16, AMODE_PLAIN, EPI_STORE>(p, (hipStream_t)stream);
    return launch_gemm_nt<ELEM_BF16, AMODE_PLAIN, EPI_STORE>(p, (hipStream_t)stream);
}

// tools/stride_microbench.py: the ping-pong NT block with operand row pitches as parameters (do power-of-two pitches cost cache channels?)
int sgc_dbg_gemm_nt_ld(const void* A, const void* B, void* C, int M, int N, int K, long lda, long ldb, void* stream) {
    NtParams p{};
    p.A = (const u16*)A; p.B = (const u16*)B; p.C = C; p.M = M; p.N = N; p.K = K;
    p.lda = lda; p.ldb = ldb; p.ldc = N; p.epi_lds = 1;
    if ((N % 256) || (K % 64) || (lda % 8) || (ldb % 8)) return SGC_ERR_ARG;
    return launch_gemm_nt_pp<ELEM_BF16, EPI_STORE>(p, (hipStream_t)stream);
}

// A: zero-padded channels-last images [n_img][S+2][S+2][Cin]; B: [N][Cin/64][9][64]; C: [n_img*S*S][N] window-major rows
int sgc_dbg_conv_nt(int elem, const void* A, const void* B, void* C, int n_img, int lgS, int Cin, int N,
                    const float* bias, void* stream) {
    NtParams p{};
    p.A = (const u16*)A; p.B = (const u16*)B; p.C = C; p.M = n_img << (2 * lgS); p.N = N; p.K = 9 * Cin;
    p.ldb = 9L * Cin; p.ldc = N; p.lgS = lgS; p.Cin = Cin; p.bias = bias;
    if (elem == ELEM_F16) return launch_gemm_nt<ELEM_F16, AMODE_CONV, EPI_STORE>(p, (hipStream_t)stream);
    return launch_gemm_nt<ELEM_BF16, AMODE_CONV, EPI_STORE>(p, (hipStream_t)stream);
}

// C slabs [splits][M][N] f32; returns number of slabs written through *slabs
int sgc_dbg_gemm_tn(int elem, const void* A, const void* B, float* C, int M, int N, int K,
                    long lda, long ldb, int splits, int* slabs, void* stream) {
    TnParams p{};
    p.A = (const u16*)A; p.B = (const u16*)B; p.C = C; p.M = M; p.N = N; p.K = K;
    p.lda = lda; p.ldb = ldb; p.ldc = N; p.slab_stride = (long)M * N;
    int r = (elem == ELEM_F16) ? launch_gemm_tn<ELEM_F16, BMODE_PLAIN>(p, splits, slabs, (hipStream_t)stream)
                               : launch_gemm_tn<ELEM_BF16, BMODE_PLAIN>(p, splits, slabs, (hipStream_t)stream);
    return r;
}

// A: [n_img*S*S][M] rows window-major; B: padded images [n_img][S+2][S+2][Cin]; C slabs [splits][M][9*Cin]
int sgc_dbg_conv_tn(int elem, const void* A, const void* B, float* C, int M, int n_img, int lgS, int Cin,
                    int splits, int* slabs, void* stream) {
    TnParams p{};
    p.A = (const u16*)A; p.B = (const u16*)B; p.C = C; p.M = M; p.N = 9 * Cin; p.K = n_img << (2 * lgS);
    p.lda = M; p.ldc = 9L * Cin; p.slab_stride = (long)M * 9 * Cin; p.lgS = lgS; p.Cin = Cin;
    int r = (elem == ELEM_F16) ? launch_gemm_tn<ELEM_F16, BMODE_CONV>(p, splits, slabs, (hipStream_t)stream)
                               : launch_gemm_tn<ELEM_BF16, BMODE_CONV>(p, splits, slabs, (hipStream_t)stream);
    return r;
}

// ds_read_b64_tr_b16 semantics probe: LDS filled with its own element index; every lane reads at byte addr[lane]
__global__ void tr_probe_kernel(const int* addr, short* out) {
    __shared__ __attribute__((aligned(16))) short lds[4096];
    for (int i = threadIdx.x; i < 4096; i += 64) lds[i] = (short)i;
    __syncthreads();
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)((char*)lds + addr[threadIdx.x]));
    for (int j = 0; j < 4; ++j) out[threadIdx.x * 4 + j] = v[j];
}
int sgc_dbg_tr_probe(const int* addr, short* out, void* stream) {
    SGC_LAUNCH(tr_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, addr, out);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

// v_mfma_f32_16x16x32_{f16,bf16} layout probe (mfma16 of gemm_nt.h): lane l passes a[l*8 .. +7] and b[l*8 .. +7]; c[l*4 + r] = register r
__global__ void mfma16_probe_kernel(const u16* a, const u16* b, float* c, int elem) {
    const int l = threadIdx.x;
    s16x8 av, bv;
    for (int i = 0; i < 8; ++i) { av[i] = (short)a[l * 8 + i]; bv[i] = (short)b[l * 8 + i]; }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = elem == ELEM_F16 ? mfma16<ELEM_F16>(av, bv, acc) : mfma16<ELEM_BF16>(av, bv, acc);
    for (int r = 0; r < 4; ++r) c[l * 4 + r] = acc[r];
}
int sgc_dbg_mfma16_probe(int elem, const void* a, const void* b, float* c, void* stream) {
    SGC_LAUNCH(mfma16_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const u16*)a, (const u16*)b, c, elem);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

// v_smfmac_f32_32x32x32_bf16 semantics probe: every lane supplies its 8 compressed A values, 16 B values and the index word
__global__ void smfmac_probe_kernel(const u16* a, const u16* b, const int* idx, float* c, int abid) {
    typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
    typedef __bf16 bf16x16_t __attribute__((ext_vector_type(16)));
    const int l = threadIdx.x;
    bf16x8_t av; bf16x16_t bv;
    for (int i = 0; i < 8; ++i) { u16 t = a[l * 8 + i]; av[i] = __builtin_bit_cast(__bf16, t); }
    for (int i = 0; i < 16; ++i) { u16 t = b[l * 16 + i]; bv[i] = __builtin_bit_cast(__bf16, t); }
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (abid == 0) acc = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(av, bv, acc, idx[l], 0, 0);
    else if (abid == 1) acc = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(av, bv, acc, idx[l], 0, 1);
    else acc = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(av, bv, acc, idx[l], 1, 0);
    for (int r = 0; r < 16; ++r) c[l * 16 + r] = acc[r];
}
int sgc_dbg_smfmac_probe(const void* a, const void* b, const int* idx, float* c, int abid, void* stream) {
    SGC_LAUNCH(smfmac_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const u16*)a, (const u16*)b, idx, c, abid);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

}  // extern "C"
// MFMA issue-rate probe: 8 independent accumulators, `iters` rounds of 8 instructions per wave; mode 0 dense 32x32x16, 1 sparse 32x32x32
template <int mode>
__global__ __launch_bounds__(512, 2) void mfma_rate_kernel(float* out, int iters) {
    typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
    typedef __bf16 bf16x16_t __attribute__((ext_vector_type(16)));
    f32x16 acc[8];
    for (int i = 0; i < 8; ++i) for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    bf16x8_t a; bf16x16_t b;
    for (int i = 0; i < 8; ++i) a[i] = (__bf16)(float)(threadIdx.x * 0.001f + i);
    for (int i = 0; i < 16; ++i) b[i] = (__bf16)(float)(threadIdx.x * 0.002f + i);
    const bf16x8_t b8 = __builtin_shufflevector(b, b, 0, 1, 2, 3, 4, 5, 6, 7);
    const int idx = 0x4444;
    for (int it = 0; it < iters; ++it) {
        if (mode == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b8, acc[i], 0, 0, 0);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(a, b, acc[i], idx, 0, 0);
        }
    }
    float s = 0.f;
    for (int i = 0; i < 8; ++i) for (int r = 0; r < 16; ++r) s += acc[i][r];
    if (s == 12345.678f) out[0] = s;
}
extern "C" {
int sgc_dbg_mfma_rate(float* out, int blocks, int iters, int mode, void* stream) {
    if (mode == 0) SGC_LAUNCH(mfma_rate_kernel<0>, dim3(blocks), dim3(512), 0, (hipStream_t)stream, out, iters);
    else SGC_LAUNCH(mfma_rate_kernel<1>, dim3(blocks), dim3(512), 0, (hipStream_t)stream, out, iters);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

}  // extern "C"
