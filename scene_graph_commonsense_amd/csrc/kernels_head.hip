// Plug-and-play hierarchical head for any input width (reference model.py:9-34 BayesianHead), forward and backward, all f32.
//
// The four nn.Linear layers of the module are packed into one W [64][D] / b [64]: rows [0, R) the three fine-relation blocks
// (fc3_1, fc3_2, fc3_3), rows R..R+2 the super logits (fc5), the rest zero.  The products run on the exact-f32 MFMA
// (v_mfma_f32_32x32x2_f32): a result is a fixed-order fmaf chain, so every output and gradient is the same bits on every run.
//
//   forward   z = h W^T + b, then super log-softmax and the three tempered log-softmaxes plus the super log-prob (model.py:25-33);
//             h is read once (the reference reads it once per nn.Linear).
//   backward  dz from the saved outputs (softmax_k = exp(rel_k - sup[k]), softmax(s) = exp(sup)), then dh = dz W and per-row-chunk
//             partials of dW = dz^T h, db = sum dz in one pass; the partials are summed by a separate fixed-order reduce.
#include "common.h"

namespace {

constexpr int ANY_WAVES = 4;          // wavefronts per workgroup (both kernels)
constexpr int ANY_BWD_ROWS = 256;     // rows of h per backward workgroup = rows per dW partial
constexpr int DZ_LD = 65;             // LDS row stride of dz [rows][64] (odd: the dh operand reads walk rows)

__device__ __forceinline__ float hmax(float v, bool in) {
    float x = in ? v : -INFINITY;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
    return x;
}
__device__ __forceinline__ float hsum(float v, bool in) {
    float x = in ? v : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// Four consecutive k of one row, zero past D.  VEC: rows are 16-byte aligned (D % 4 == 0), so four k are all in or all out.
template <bool VEC>
__device__ __forceinline__ f32x4 ld4(const float* row, int k, int D) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
        if (k < D) v = *reinterpret_cast<const f32x4*>(row + k);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (k + j < D) v[j] = row[k + j];
    }
    return v;
}

struct AnyFwdParams {
    const float* h; const float* W; const float* b; int M; int D; int ng, np, ns; float T1, T2, T3; float* rel; float* sup;
};

// One workgroup per tile of TM*32 rows.  Wave w takes the k-chunks c = w, w+4, ... of 8 k: lane (i, half) loads h[row i][8c+4half ..
// +3] and W[n][8c+4half .. +3] as one 16-byte vector each and issues four MFMAs per (row tile, 32 outputs) - the k order inside a
// chunk is the same permutation for both operands.  The four waves' partial sums meet in LDS and are added in wave order.
template <int TM, bool VEC>
__global__ __launch_bounds__(256) void head_any_fwd_kernel(const AnyFwdParams p) {
    __shared__ float red[ANY_WAVES][TM * 32][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const long m0 = (long)blockIdx.x * (TM * 32);
    const int D = p.D;
    const float* hrow[TM];
#pragma unroll
    for (int t = 0; t < TM; ++t) {
        const long r = m0 + t * 32 + li;                    // rows past M read row M-1 and are not written
        hrow[t] = p.h + (r < p.M ? r : (long)p.M - 1) * D;
    }
    const float* wrow0 = p.W + (long)li * D;
    const float* wrow1 = p.W + (long)(32 + li) * D;
    f32x16 acc[TM][2];
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][0][i] = acc[t][1][i] = 0.f;

    const int nchunk = (D + 7) >> 3;
    int c = w;
    f32x4 a[TM], b0, b1;
#pragma unroll
    for (int t = 0; t < TM; ++t) a[t] = ld4<VEC>(hrow[t], c * 8 + lh * 4, D);
    b0 = ld4<VEC>(wrow0, c * 8 + lh * 4, D);
    b1 = ld4<VEC>(wrow1, c * 8 + lh * 4, D);
    while (c < nchunk) {                                    // one chunk in flight ahead of the MFMAs (past the end: zeros, no load)
        const int cn = c + ANY_WAVES;
        f32x4 an[TM];
#pragma unroll
        for (int t = 0; t < TM; ++t) an[t] = ld4<VEC>(hrow[t], cn * 8 + lh * 4, D);
        const f32x4 bn0 = ld4<VEC>(wrow0, cn * 8 + lh * 4, D), bn1 = ld4<VEC>(wrow1, cn * 8 + lh * 4, D);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < TM; ++t) {
                acc[t][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][j], b0[j], acc[t][0], 0, 0, 0);
                acc[t][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][j], b1[j], acc[t][1], 0, 0, 0);
            }
#pragma unroll
        for (int t = 0; t < TM; ++t) a[t] = an[t];
        b0 = bn0; b1 = bn1; c = cn;
    }
    // C/D map of the 32x32 f32 MFMA: column = lane & 31 (output), row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5) (row of h)
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = t * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
            red[w][r][li] = acc[t][0][i];
            red[w][r][32 + li] = acc[t][1][i];
        }
    __syncthreads();

    // epilogue: one wavefront per row, lane = output row of W
    const int R = p.ng + p.np + p.ns;
    const float bias = p.b[lane];
    const bool in_sup = lane >= R && lane < R + 3;
    const int seg = lane < p.ng ? 0 : (lane < p.ng + p.np ? 1 : 2);
    const float T = seg == 0 ? p.T1 : (seg == 1 ? p.T2 : p.T3);
    for (int rr = w; rr < TM * 32; rr += ANY_WAVES) {
        const long m = m0 + rr;
        if (m >= p.M) break;                                // wave-uniform
        const float z = (((red[0][rr][lane] + red[1][rr][lane]) + red[2][rr][lane]) + red[3][rr][lane]) + bias;
        const float smax = hmax(z, in_sup);
        const float ssum = hsum(expf(z - smax), in_sup);
        const float slog = z - smax - logf(ssum);          // valid on the three super lanes
        if (in_sup) p.sup[m * 3 + (lane - R)] = slog;
        const float x = z / T;
        float out = 0.f;
#pragma unroll
        for (int sg = 0; sg < 3; ++sg) {
            const bool in = lane < R && seg == sg;
            const float mx = hmax(x, in);
            const float sm = hsum(expf(x - mx), in);
            const float sl = __shfl(slog, R + sg);
            if (in) out = x - mx - logf(sm) + sl;
        }
        if (lane < R) p.rel[m * R + lane] = out;
    }
}

struct AnyBwdParams {
    const float* h; const float* W; const float* rel; const float* sup; const float* g_rel; const float* g_sup;
    int M; int D; int ng, np, ns; float T1, T2, T3; float* dh; float* part;
};

// Workgroup (x, y): rows [256x, 256x + 256) of h, 32-column blocks y*4 + w, y*4 + w + 4*gridDim.y, ... of D for wave w.
// Stage 1 writes dz [256][64] (dL/dz of the packed logits) to LDS from the saved outputs and the upstream gradients; stage 2 per
// column block: dh[rows][block] = dz W[:, block] (K = 64, the W operands stay in registers over the row tiles) and
// dW[:, block] += dz^T h[rows][block] (K = the rows), kept in registers until the block's partial is written.  Workgroup (x, 0)
// also writes db's partial, sum dz over its rows in row order.  part [gridDim.x][64][D+1], column D = db.
__global__ __launch_bounds__(256) void head_any_bwd_kernel(const AnyBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* dzs = reinterpret_cast<float*>(smem);            // [ANY_BWD_ROWS][DZ_LD]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const long r0 = (long)blockIdx.x * ANY_BWD_ROWS;
    const int D = p.D;
    const int R = p.ng + p.np + p.ns;

    const bool fine = lane < R, in_sup = lane >= R && lane < R + 3;
    const int seg = lane < p.ng ? 0 : (lane < p.ng + p.np ? 1 : 2);
    const float T = seg == 0 ? p.T1 : (seg == 1 ? p.T2 : p.T3);
    const int ks = in_sup ? lane - R : 0;
    for (int i = w; i < ANY_BWD_ROWS; i += ANY_WAVES) {
        const long m = r0 + i;
        float v = 0.f;
        if (m < p.M) {                                      // wave-uniform
            const float g = (fine && p.g_rel) ? p.g_rel[m * R + lane] : 0.f;
            const float gs0 = hsum(g, fine && seg == 0), gs1 = hsum(g, fine && seg == 1), gs2 = hsum(g, fine && seg == 2);
            if (fine) v = (g - expf(p.rel[m * R + lane] - p.sup[m * 3 + seg]) * (seg == 0 ? gs0 : (seg == 1 ? gs1 : gs2))) / T;
            const float G = (in_sup && p.g_sup ? p.g_sup[m * 3 + ks] : 0.f) + (ks == 0 ? gs0 : (ks == 1 ? gs1 : gs2));
            const float SG = hsum(G, in_sup);
            if (in_sup) v = G - expf(p.sup[m * 3 + ks]) * SG;
        }
        dzs[i * DZ_LD + lane] = v;                          // rows past M: zero, so they add nothing to dW / db
    }
    __syncthreads();
    if (p.part && blockIdx.y == 0 && w == 0) {
        float s = 0.f;
        for (int i = 0; i < ANY_BWD_ROWS; ++i) s += dzs[i * DZ_LD + lane];
        p.part[((long)blockIdx.x * 64 + lane) * (D + 1) + D] = s;
    }

    const long rows = (long)p.M - r0 < ANY_BWD_ROWS ? (long)p.M - r0 : ANY_BWD_ROWS;
    const int ntile = (int)((rows + 31) / 32);
    const int nblk = (D + 31) / 32;
    for (int blk = blockIdx.y * ANY_WAVES + w; blk < nblk; blk += gridDim.y * ANY_WAVES) {
        const int d = blk * 32 + li;
        const bool din = d < D;
        float wb[32];
        if (p.dh) {
#pragma unroll
            for (int s = 0; s < 32; ++s) wb[s] = din ? p.W[(long)(2 * s + lh) * D + d] : 0.f;
        }
        f32x16 aw0, aw1;
#pragma unroll
        for (int i = 0; i < 16; ++i) aw0[i] = aw1[i] = 0.f;
        for (int t = 0; t < ntile; ++t) {
            const float* dzt = dzs + t * 32 * DZ_LD;
            if (p.dh) {
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
                for (int s = 0; s < 32; ++s)          // A[row li][k = output 2s + lh], B[k][column d]
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dzt[li * DZ_LD + 2 * s + lh], wb[s], acc, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const long m = r0 + t * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
                    if (m < p.M && din) p.dh[m * D + d] = acc[i];
                }
            }
            if (p.part) {
                float hb[16];
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const long m = r0 + t * 32 + 2 * s + lh;
                    hb[s] = (m < p.M && din) ? p.h[m * D + d] : 0.f;
                }
#pragma unroll
                for (int s = 0; s < 16; ++s) {        // A[output li (+32)][k = row 2s + lh], B[k][column d]
                    const float* zr = dzt + (2 * s + lh) * DZ_LD;
                    aw0 = __builtin_amdgcn_mfma_f32_32x32x2f32(zr[li], hb[s], aw0, 0, 0, 0);
                    aw1 = __builtin_amdgcn_mfma_f32_32x32x2f32(zr[32 + li], hb[s], aw1, 0, 0, 0);
                }
            }
        }
        if (p.part && din) {
            float* pb = p.part + (long)blockIdx.x * 64 * (D + 1) + d;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int o = (i & 3) + 8 * (i >> 2) + 4 * lh;
                pb[(long)o * (D + 1)] = aw0[i];
                pb[(long)(32 + o) * (D + 1)] = aw1[i];
            }
        }
    }
}

// out[e] = sum over q = 0 .. n_part-1 of part[q][e], q ascending: the same bits on every run, no atomics.
__global__ __launch_bounds__(256) void head_any_wreduce_kernel(const float* part, int n_part, long n, float* out) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        float s = 0.f;
#pragma unroll 8
        for (int q = 0; q < n_part; ++q) s += part[(long)q * n + e];
        out[e] = s;
    }
}

}  // namespace

extern "C" {

int sgc_bayes_head_any(const float* h, const float* W, const float* bias, int M, int D, int ng, int np, int ns, float T1, float T2,
                       float T3, float* rel, float* sup, void* stream) {
    if (D < 1 || M < 0 || ng < 0 || np < 0 || ns < 0 || ng + np + ns + 3 > 64) return SGC_ERR_ARG;
    if (M == 0) return SGC_OK;
    const AnyFwdParams p{h, W, bias, M, D, ng, np, ns, T1, T2, T3, rel, sup};
    const bool vec = D % 4 == 0 && ((uintptr_t)h & 15) == 0 && ((uintptr_t)W & 15) == 0;
    // 64-row tiles halve the W traffic once there are enough of them to fill the chip; 32-row tiles below that
    if (M >= 32768) {
        const dim3 grid((M + 63) / 64);
        if (vec) SGC_LAUNCH((head_any_fwd_kernel<2, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
        else SGC_LAUNCH((head_any_fwd_kernel<2, false>), grid, dim3(256), 0, (hipStream_t)stream, p);
    } else {
        const dim3 grid((M + 31) / 32);
        if (vec) SGC_LAUNCH((head_any_fwd_kernel<1, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
        else SGC_LAUNCH((head_any_fwd_kernel<1, false>), grid, dim3(256), 0, (hipStream_t)stream, p);
    }
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

int sgc_bayes_head_any_bwd(const float* h, const float* W, const float* rel, const float* sup, const float* g_rel, const float* g_sup,
                           int M, int D, int ng, int np, int ns, float T1, float T2, float T3, float* dh, float* part, void* stream) {
    if (D < 1 || M < 0 || ng < 0 || np < 0 || ns < 0 || ng + np + ns + 3 > 64) return SGC_ERR_ARG;
    if (M == 0 || (!dh && !part)) return SGC_OK;
    const AnyBwdParams p{h, W, rel, sup, g_rel, g_sup, M, D, ng, np, ns, T1, T2, T3, dh, part};
    const int nx = (M + ANY_BWD_ROWS - 1) / ANY_BWD_ROWS;
    const int nquad = (D + 32 * ANY_WAVES - 1) / (32 * ANY_WAVES);       // 128-column groups of D
    int ny = (512 + nx - 1) / nx;                                         // about two workgroups per CU
    if (ny > nquad) ny = nquad;
    const int lds = ANY_BWD_ROWS * DZ_LD * 4;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(head_any_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    SGC_LAUNCH(head_any_bwd_kernel, dim3(nx, ny), dim3(256), lds, (hipStream_t)stream, p);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

int sgc_bayes_head_any_wreduce(const float* part, int n_part, int D, float* out, void* stream) {
    if (D < 1 || n_part < 0) return SGC_ERR_ARG;
    const long n = 64L * (D + 1);
    long blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    SGC_LAUNCH(head_any_wreduce_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, part, n_part, n, out);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

}  // extern "C"
