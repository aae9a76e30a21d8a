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
//
// The forward's main loop has two more epilogues on the same logit bits: the class-weighted hierarchical NLL (train_utils.py:116-157)
// with dz = dL/dz formed straight from the logits, which the backward then reads from memory instead of rebuilding it, and the three
// ranked candidates per row (evaluator.py:160-174).
//
// Commonsense (run modes train_cs / eval_cs) rides on the same main loop.  EPI_LOSS_CS adds the penalty of train_utils.py:36-60 to
// the loss epilogue: per row and block the largest softmax value p, its first arg-max and the two triplet-set lookups; the penalty's
// normalisers (the numbers of flagged candidates) are known only after every row, so the forward leaves the un-normalised direction
// dp/dz, the flags and per-workgroup partials, a fixed-order sum forms the normalisers, and stage 1 of the backward reads
// g (dz + c dir).  EPI_CAND_CS is EPI_CAND with the filter of evaluator.py:189-194 on each slot.
#include "common.h"
#include "eval_geom.h"

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
    // EPI_LOSS: target [M] (int64 when tgt64, else int32), cw [R] or null, norm [4], dz [M][64] or null, loss_part [gridDim.x]
    const void* target; int tgt64; const float* cw; const float* norm; float* dz; double* loss_part;
    // EPI_CAND: cand_conf / cand_pred [M][3] (sup is written too)
    float* cand_conf; int* cand_pred;
    // EPI_LOSS_CS / EPI_CAND_CS: categories [M] (int64 when cat64, else int32) and the two triplet bitmaps over C x R x C
    const void* scat; const void* ocat; int cat64; const unsigned* aligned; const unsigned* violated; int C;
    // EPI_LOSS_CS: dir [M][64] or null, flags [M][3] or null (bit 0 weak, bit 1 strong), cs_part [2][gridDim.x], cs_cnt [2][gridDim.x]
    float* dir; unsigned char* flags; double* cs_part; int* cs_cnt;
};

enum { EPI_LOGPROB = 0, EPI_LOSS = 1, EPI_CAND = 2, EPI_LOSS_CS = 3, EPI_CAND_CS = 4 };
constexpr bool epi_loss(int e) { return e == EPI_LOSS || e == EPI_LOSS_CS; }
constexpr bool epi_cand(int e) { return e == EPI_CAND || e == EPI_CAND_CS; }

// Row m's target, or -1 for a row the loss skips (negative = "no relation"; a value past R is skipped too, never indexed with).
__device__ __forceinline__ int head_target(const void* target, int tgt64, long m, int R) {
    const long long t = tgt64 ? static_cast<const long long*>(target)[m] : static_cast<const int*>(target)[m];
    return (t >= 0 && t < R) ? (int)t : -1;
}
__device__ __forceinline__ long head_category(const void* cat, int cat64, long m) {
    return cat64 ? (long)static_cast<const long long*>(cat)[m] : (long)static_cast<const int*>(cat)[m];
}

// One workgroup per tile of TM*32 rows.  Wave w takes the k-chunks c = w, w+4, ... of 8 k: lane (i, half) loads h[row i][8c+4half ..
// +3] and W[n][8c+4half .. +3] as one 16-byte vector each and issues four MFMAs per (row tile, 32 outputs) - the k order inside a
// chunk is the same permutation for both operands.  The four waves' partial sums meet in LDS and are added in wave order.
// EPI selects what is made of the logits: the module's four log-prob outputs, the hierarchical loss and its dz, or the candidates.
template <int TM, bool VEC, int EPI>
__global__ __launch_bounds__(256) void head_any_fwd_kernel(const AnyFwdParams p) {
    __shared__ __attribute__((aligned(16))) float red[ANY_WAVES][TM * 32][64];
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
    double lsum = 0.0;                                      // EPI_LOSS: this wave's loss terms, in row order
    double pw = 0.0, ps = 0.0;                              // EPI_LOSS_CS: lane k < 3: sums of p over the weak / strong candidates of
    int nw = 0, nst = 0;                                    //              block k in this wave's rows, and their numbers
    float inv_c = 0.f, wsum[3] = {1.f, 1.f, 1.f};
    if (epi_loss(EPI) && p.target) {                        // no target table (EPI_LOSS_CS only): the penalty alone
        inv_c = p.norm[0] > 0.f ? 1.f / p.norm[0] : 0.f;
        wsum[0] = p.norm[1]; wsum[1] = p.norm[2]; wsum[2] = p.norm[3];
    }
    for (int rr = w; rr < TM * 32; rr += ANY_WAVES) {
        const long m = m0 + rr;
        if (m >= p.M) break;                                // wave-uniform
        const float z = (((red[0][rr][lane] + red[1][rr][lane]) + red[2][rr][lane]) + red[3][rr][lane]) + bias;
        const float smax = hmax(z, in_sup);
        const float ssum = hsum(expf(z - smax), in_sup);
        if (epi_loss(EPI)) {
            // L = a * -sup[k] + b * -rel_k[t - off_k] with a = 1/|C|, b = w[t] / sum_{C_k} w (train_utils.py:131-151), so
            // dz_sup = (a + b)(softmax(z_sup) - e_k), dz_k = (b / T_k)(softmax(z_k / T_k) - e_t), everything else zero
            const int t = (EPI == EPI_LOSS || p.target) ? head_target(p.target, p.tgt64, m, R) : -1;    // wave-uniform
            float v = 0.f;
            if (t >= 0) {
                const int k = t < p.ng ? 0 : (t < p.ng + p.np ? 1 : 2);
                const float a = inv_c, b = (p.cw ? p.cw[t] : 1.f) / (k == 0 ? wsum[0] : (k == 1 ? wsum[1] : wsum[2]));
                const float slog = __shfl(z - smax - logf(ssum), R + k);
                const bool in = lane < R && seg == k;
                const float x = z / T;
                const float mx = hmax(x, in);
                const float e = expf(x - mx);
                const float sm = hsum(e, in);
                const float rel_t = __shfl(x - mx - logf(sm) + slog, t);       // the value forward() gives at the target
                if (in) v = (b / T) * (e / sm - (lane == t ? 1.f : 0.f));
                if (in_sup) v = (a + b) * (expf(z - smax) / ssum - (lane - R == k ? 1.f : 0.f));
                lsum += (double)(-(a * slog) - b * rel_t);
            }
            if (p.dz) p.dz[m * 64 + lane] = v;
            if (EPI == EPI_LOSS) continue;
        }
        if (EPI == EPI_LOSS_CS) {
            // train_utils.py:36-60 for every row: per block p = max softmax(z_k / T_k) = 1 / sm, pred = the first arg-max as
            // EPI_CAND finds it (same operations, same bits), weak = (s, pred, o) not aligned, strong = violated.  The gradient
            // goes through p only: dp/dz_j = p ([j == pred] - softmax_j) / T_k, written without the normaliser.
            const long sc = head_category(p.scat, p.cat64, m), oc = head_category(p.ocat, p.cat64, m);      // wave-uniform
            const float slog = z - smax - logf(ssum);
            const float x = z / T;
            float dv = 0.f, mypm = 0.f;
            int mypred = 0;                                 // lane k < 3 keeps block k's predicate and p
#pragma unroll
            for (int sg = 0; sg < 3; ++sg) {
                const bool in = lane < R && seg == sg;
                const float mx = hmax(x, in);
                const float e = expf(x - mx);
                const float sm = hsum(e, in);
                const float sl = __shfl(slog, R + sg);
                const float out = x - mx - logf(sm) + sl;
                const float best = 0.f - logf(sm) + sl;
                const unsigned long long hit = __ballot(in && out == best);
                const int pred = hit ? __ffsll(hit) - 1 : (sg == 0 ? 0 : (sg == 1 ? p.ng : p.ng + p.np));
                const float pm = 1.f / sm;
                if (lane == sg) { mypred = pred; mypm = pm; }
                if (in) dv = pm * ((lane == pred ? 1.f : 0.f) - e / sm) / T;
            }
            // the three lookups of the row as one load per set on lanes 0..2 (one memory latency per row, not three in a chain)
            const unsigned bits = lane < 3 ? triplet_bits(p.aligned, p.violated, sc, mypred, oc, p.C, R) : 1u;
            if (!(bits & 1u)) { pw += (double)mypm; ++nw; }                // lane k: block k's candidates of this wave's rows
            if (bits & 2u) { ps += (double)mypm; ++nst; }
            if (p.dir) p.dir[m * 64 + lane] = dv;
            if (p.flags && lane < 3) p.flags[m * 3 + lane] = (unsigned char)((bits & 2u) | ((bits & 1u) ^ 1u));
            continue;
        }
        const float slog = z - smax - logf(ssum);          // valid on the three super lanes
        if (in_sup) p.sup[m * 3 + (lane - R)] = slog;
        const float x = z / T;
        float out = 0.f, cbest = 0.f;
        int cpred = 0;
#pragma unroll
        for (int sg = 0; sg < 3; ++sg) {
            const bool in = lane < R && seg == sg;
            const float mx = hmax(x, in);
            const float sm = hsum(expf(x - mx), in);
            const float sl = __shfl(slog, R + sg);
            if (in) out = x - mx - logf(sm) + sl;
            if (epi_cand(EPI)) {
                // evaluator.py:160-174: the block's maximum and its first arg-max.  out rises with x, so its maximum is out where
                // x == mx, the same operations on x - mx = 0: no second reduction.  Lanes of equal out may differ in x: ballot on out.
                const float best = 0.f - logf(sm) + sl;
                const unsigned long long hit = __ballot(in && out == best);
                if (lane == sg) {
                    cbest = best;
                    cpred = hit ? __ffsll(hit) - 1 : (sg == 0 ? 0 : (sg == 1 ? p.ng : p.ng + p.np));
                    if (EPI == EPI_CAND_CS) {               // evaluator.py:189-194: keep = aligned and not violated
                        const long sc = head_category(p.scat, p.cat64, m), oc = head_category(p.ocat, p.cat64, m);
                        if (triplet_bits(p.aligned, p.violated, sc, cpred, oc, p.C, R) != 1u) cbest = -INFINITY;
                    }
                }
            }
        }
        if (epi_cand(EPI) && lane < 3) {
            p.cand_conf[m * 3 + lane] = cbest;
            p.cand_pred[m * 3 + lane] = cpred;
        }
        if (EPI == EPI_LOGPROB && lane < R) p.rel[m * R + lane] = out;
    }
    if (epi_loss(EPI)) {                                    // one partial per workgroup: the four waves' sums in wave order
        __syncthreads();                                    // red is read no more
        double* ws = reinterpret_cast<double*>(&red[0][0][0]);
        int* wn = reinterpret_cast<int*>(ws + 3 * ANY_WAVES);
        if (EPI == EPI_LOSS_CS) {                           // the three blocks' lanes in block order
            pw = (__shfl(pw, 0) + __shfl(pw, 1)) + __shfl(pw, 2);
            ps = (__shfl(ps, 0) + __shfl(ps, 1)) + __shfl(ps, 2);
            nw = (__shfl(nw, 0) + __shfl(nw, 1)) + __shfl(nw, 2);
            nst = (__shfl(nst, 0) + __shfl(nst, 1)) + __shfl(nst, 2);
        }
        if (lane == 0) {
            ws[w] = lsum;
            if (EPI == EPI_LOSS_CS) { ws[ANY_WAVES + w] = pw; ws[2 * ANY_WAVES + w] = ps; wn[w] = nw; wn[ANY_WAVES + w] = nst; }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            p.loss_part[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
            if (EPI == EPI_LOSS_CS) {
                p.cs_part[blockIdx.x] = ((ws[4] + ws[5]) + ws[6]) + ws[7];
                p.cs_part[gridDim.x + blockIdx.x] = ((ws[8] + ws[9]) + ws[10]) + ws[11];
                p.cs_cnt[blockIdx.x] = ((wn[0] + wn[1]) + wn[2]) + wn[3];
                p.cs_cnt[gridDim.x + blockIdx.x] = ((wn[4] + wn[5]) + wn[6]) + wn[7];
            }
        }
    }
}

// norm[0] = |C| (rows with a target in [0, R)), norm[1..3] = sum of w[target] over the rows of each block.  One workgroup: thread i
// adds rows i, i + 1024, ... in order, then a fixed tree over the threads, all in double - the same bits on every run.
__global__ __launch_bounds__(1024) void head_loss_norm_kernel(const void* target, int tgt64, const float* cw, int M, int ng, int np,
                                                              int ns, float* norm) {
    __shared__ double acc[4][1024];
    const int R = ng + np + ns;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long m = threadIdx.x; m < M; m += 1024) {
        const int t = head_target(target, tgt64, m, R);
        if (t >= 0) {
            s[0] += 1.0;
            s[t < ng ? 1 : (t < ng + np ? 2 : 3)] += (double)(cw ? cw[t] : 1.f);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q][threadIdx.x] = s[q];
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q][threadIdx.x] += acc[q][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < 4) norm[threadIdx.x] = (float)acc[threadIdx.x][0];
}

// loss = sum of the n workgroup partials: thread i adds partials i, i + 256, ... in order, then a fixed tree, in double.
__global__ __launch_bounds__(256) void head_loss_sum_kernel(const double* part, int n, float* loss) {
    __shared__ double acc[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += part[i];
    acc[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) acc[threadIdx.x] += acc[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)acc[0];
}

// The commonsense call's scalars from the n workgroup partials, in the order of head_loss_sum_kernel: N_w, N_s (cnt_out [2], int64),
// out[0] = nll + lambda_cs * penalty, out[1] = nll, out[2] = penalty = [N_w > 0] lambda_weak * sum_w / N_w + [N_s > 0] lambda_strong
// * sum_s / N_s (train_utils.py:56-60), and the backward's coefficients out[3] = lambda_cs * lambda_weak / N_w, out[4] = lambda_cs
// * lambda_strong / N_s (0 where the count is 0).
__global__ __launch_bounds__(256) void head_cs_sum_kernel(const double* loss_part, const double* cs_part, const int* cs_cnt, int n,
                                                          float lambda_cs, float lambda_weak, float lambda_strong, float* out,
                                                          long long* cnt_out) {
    __shared__ double acc[3][256];
    __shared__ long long cnt[2][256];
    double s[3] = {0.0, 0.0, 0.0};
    long long c[2] = {0, 0};
    for (int i = threadIdx.x; i < n; i += 256) {
        s[0] += loss_part[i]; s[1] += cs_part[i]; s[2] += cs_part[n + i];
        c[0] += cs_cnt[i]; c[1] += cs_cnt[n + i];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[q][threadIdx.x] = s[q];
    cnt[0][threadIdx.x] = c[0]; cnt[1][threadIdx.x] = c[1];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[q][threadIdx.x] += acc[q][threadIdx.x + o];
            cnt[0][threadIdx.x] += cnt[0][threadIdx.x + o]; cnt[1][threadIdx.x] += cnt[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const long long n_w = cnt[0][0], n_s = cnt[1][0];
        const float nll = (float)acc[0][0];
        const double pen_w = n_w > 0 ? (double)lambda_weak * acc[1][0] / (double)n_w : 0.0;
        const double pen_s = n_s > 0 ? (double)lambda_strong * acc[2][0] / (double)n_s : 0.0;
        const float pen = (float)(pen_w + pen_s);
        out[0] = nll + lambda_cs * pen; out[1] = nll; out[2] = pen;
        out[3] = n_w > 0 ? (float)((double)lambda_cs * (double)lambda_weak / (double)n_w) : 0.f;
        out[4] = n_s > 0 ? (float)((double)lambda_cs * (double)lambda_strong / (double)n_s) : 0.f;
        cnt_out[0] = n_w; cnt_out[1] = n_s;
    }
}

struct AnyBwdParams {
    const float* h; const float* W; const float* rel; const float* sup; const float* g_rel; const float* g_sup;
    int M; int D; int ng, np, ns; float T1, T2, T3; float* dh; float* part;
    const float* dz; const float* g;                        // FROM_DZ: dz [M][64] of the loss forward, g = the scalar dL/d(loss)
    // FROM_DZ_CS: dz may be null (= zero); dir [M][64], flags [M][3] of the commonsense forward, coef [2] = lambda_cs lambda_weak /
    // N_w, lambda_cs lambda_strong / N_s
    const float* dir; const unsigned char* flags; const float* coef;
};

enum { FROM_OUTPUTS = 0, FROM_DZ = 1, FROM_DZ_CS = 2 };

// Workgroup (x, y): rows [256x, 256x + 256) of h, 32-column blocks y*4 + w, y*4 + w + 4*gridDim.y, ... of D for wave w.
// Stage 1 writes dz [256][64] (dL/dz of the packed logits) to LDS from the saved outputs and the upstream gradients; stage 2 per
// column block: dh[rows][block] = dz W[:, block] (K = 64, the W operands stay in registers over the row tiles) and
// dW[:, block] += dz^T h[rows][block] (K = the rows), kept in registers until the block's partial is written.  Workgroup (x, 0)
// also writes db's partial, sum dz over its rows in row order.  part [gridDim.x][64][D+1], column D = db.
// FROM_DZ: stage 1 is a copy of g * dz from memory (the fused loss formed dz in its forward).  FROM_DZ_CS: of g * (dz + c * dir) with
// c = coef[0] weak + coef[1] strong of the row's block - the commonsense penalty's normalisers enter here, after the forward.
template <int SRC>
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
    const float gl = SRC != FROM_OUTPUTS ? *p.g : 0.f;
    const float cf_w = SRC == FROM_DZ_CS ? p.coef[0] : 0.f, cf_s = SRC == FROM_DZ_CS ? p.coef[1] : 0.f;
    for (int i = w; i < ANY_BWD_ROWS; i += ANY_WAVES) {
        const long m = r0 + i;
        float v = 0.f;
        if (SRC == FROM_DZ) {
            if (m < p.M) v = gl * p.dz[m * 64 + lane];
        } else if (SRC == FROM_DZ_CS) {
            if (m < p.M) {
                float d = p.dz ? p.dz[m * 64 + lane] : 0.f;
                if (fine) {
                    const unsigned f = p.flags[m * 3 + seg];
                    const float c = ((f & 1u) ? cf_w : 0.f) + ((f & 2u) ? cf_s : 0.f);
                    d += c * p.dir[m * 64 + lane];
                }
                v = gl * d;
            }
        } else if (m < p.M) {                               // wave-uniform
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

// 64-row tiles halve the W traffic once there are enough of them to fill the chip; 32-row tiles below that
inline int any_fwd_tile(int M) { return M >= 32768 ? 64 : 32; }

template <int EPI>
int launch_any_fwd(const AnyFwdParams& p, hipStream_t stream) {
    const bool vec = p.D % 4 == 0 && ((uintptr_t)p.h & 15) == 0 && ((uintptr_t)p.W & 15) == 0;
    const int tile = any_fwd_tile(p.M);
    const dim3 grid((p.M + tile - 1) / tile);
    if (tile == 64) {
        if (vec) SGC_LAUNCH((head_any_fwd_kernel<2, true, EPI>), grid, dim3(256), 0, stream, p);
        else SGC_LAUNCH((head_any_fwd_kernel<2, false, EPI>), grid, dim3(256), 0, stream, p);
    } else {
        if (vec) SGC_LAUNCH((head_any_fwd_kernel<1, true, EPI>), grid, dim3(256), 0, stream, p);
        else SGC_LAUNCH((head_any_fwd_kernel<1, false, EPI>), grid, dim3(256), 0, stream, p);
    }
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

}  // namespace

extern "C" {


int sgc_bayes_head_any(const float* h, const float* W, const float* bias, int M, int D, int ng, int np, int ns, float T1, float T2,
                       float T3, float* rel, float* sup, void* stream) {
    if (D < 1 || M < 0 || ng < 0 || np < 0 || ns < 0 || ng + np + ns + 3 > 64) return SGC_ERR_ARG;
    if (M == 0) return SGC_OK;
    AnyFwdParams p{};
    p.h = h; p.W = W; p.b = bias; p.M = M; p.D = D; p.ng = ng; p.np = np; p.ns = ns; p.T1 = T1; p.T2 = T2; p.T3 = T3;
    p.rel = rel; p.sup = sup;
    return launch_any_fwd<EPI_LOGPROB>(p, (hipStream_t)stream);
}

int sgc_bayes_head_any_candidates(const float* h, const float* W, const float* bias, int M, int D, int ng, int np, int ns, float T1,
                                  float T2, float T3, float* cand_conf, int* cand_pred, float* sup, void* stream) {
    if (D < 1 || M < 0 || ng < 0 || np < 0 || ns < 0 || ng + np + ns + 3 > 64) return SGC_ERR_ARG;
    if (M == 0) return SGC_OK;
    if (!cand_conf || !cand_pred || !sup) return SGC_ERR_ARG;
    AnyFwdParams p{};
    p.h = h; p.W = W; p.b = bias; p.M = M; p.D = D; p.ng = ng; p.np = np; p.ns = ns; p.T1 = T1; p.T2 = T2; p.T3 = T3;
    p.sup = sup; p.cand_conf = cand_conf; p.cand_pred = cand_pred;
    return launch_any_fwd<EPI_CAND>(p, (hipStream_t)stream);
}

int sgc_bayes_head_any_loss(const float* h, const float* W, const float* bias, const void* target, int target_is_int64,
                            const float* class_weight, int M, int D, int ng, int np, int ns, float T1, float T2, float T3, float* norm,
                            float* dz, double* loss_part, float* loss, void* stream) {
    if (D < 1 || M < 0 || ng < 0 || np < 0 || ns < 0 || ng + np + ns + 3 > 64) return SGC_ERR_ARG;
    if (!norm || !loss || (M > 0 && (!target || !loss_part))) return SGC_ERR_ARG;
    SGC_LAUNCH(head_loss_norm_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, target, target_is_int64, class_weight, M, ng, np, ns,
               norm);
    SGC_CHECK_LAUNCH();
    int n_part = 0;
    if (M > 0) {
        AnyFwdParams p{};
        p.h = h; p.W = W; p.b = bias; p.M = M; p.D = D; p.ng = ng; p.np = np; p.ns = ns; p.T1 = T1; p.T2 = T2; p.T3 = T3;
        p.target = target; p.tgt64 = target_is_int64; p.cw = class_weight; p.norm = norm; p.dz = dz; p.loss_part = loss_part;
        n_part = (M + any_fwd_tile(M) - 1) / any_fwd_tile(M);      // one partial per workgroup; at most ceil(M / 32)
        const int rc = launch_any_fwd<EPI_LOSS>(p, (hipStream_t)stream);
        if (rc != SGC_OK) return rc;
    }
    SGC_LAUNCH(head_loss_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, loss_part, n_part, loss);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

int sgc_bayes_head_any_loss_bwd(const float* h, const float* W, const float* dz, const float* g, int M, int D, float* dh, float* part,
                                void* stream) {
    if (D < 1 || M < 0) return SGC_ERR_ARG;
    if (M == 0 || (!dh && !part)) return SGC_OK;
    if (!dz || !g) return SGC_ERR_ARG;
    AnyBwdParams p{};
    p.h = h; p.W = W; p.M = M; p.D = D; p.dh = dh; p.part = part; p.dz = dz; p.g = g;
    const int nx = (M + ANY_BWD_ROWS - 1) / ANY_BWD_ROWS;
    const int nquad = (D + 32 * ANY_WAVES - 1) / (32 * ANY_WAVES);
    int ny = (512 + nx - 1) / nx;
    if (ny > nquad) ny = nquad;
    const int lds = ANY_BWD_ROWS * DZ_LD * 4;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(head_any_bwd_kernel<FROM_DZ>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    SGC_LAUNCH(head_any_bwd_kernel<FROM_DZ>, dim3(nx, ny), dim3(256), lds, (hipStream_t)stream, p);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

int sgc_bayes_head_any_candidates_cs(const float* h, const float* W, const float* bias, const void* subject_cat, const void* object_cat,
                                     int cat_is_int64, const unsigned* aligned, const unsigned* violated, int C, int M, int D, int ng,
                                     int np, int ns, float T1, float T2, float T3, float* cand_conf, int* cand_pred, float* sup,
                                     void* stream) {
    if (D < 1 || M < 0 || C < 1 || ng < 0 || np < 0 || ns < 0 || ng + np + ns + 3 > 64) return SGC_ERR_ARG;
    if (M == 0) return SGC_OK;
    if (!cand_conf || !cand_pred || !sup || !subject_cat || !object_cat || !aligned || !violated) return SGC_ERR_ARG;
    AnyFwdParams p{};
    p.h = h; p.W = W; p.b = bias; p.M = M; p.D = D; p.ng = ng; p.np = np; p.ns = ns; p.T1 = T1; p.T2 = T2; p.T3 = T3;
    p.sup = sup; p.cand_conf = cand_conf; p.cand_pred = cand_pred;
    p.scat = subject_cat; p.ocat = object_cat; p.cat64 = cat_is_int64; p.aligned = aligned; p.violated = violated; p.C = C;
    return launch_any_fwd<EPI_CAND_CS>(p, (hipStream_t)stream);
}

int sgc_bayes_head_any_loss_cs(const float* h, const float* W, const float* bias, const void* target, int target_is_int64,
                               const float* class_weight, const void* subject_cat, const void* object_cat, int cat_is_int64,
                               const unsigned* aligned, const unsigned* violated, int C, int M, int D, int ng, int np, int ns, float T1,
                               float T2, float T3, float lambda_cs, float lambda_weak, float lambda_strong, float* norm, float* dz,
                               float* dir, unsigned char* flags, double* part, int* cnt_part, float* out, long long* counts,
                               void* stream) {
    if (D < 1 || M < 0 || C < 1 || ng < 0 || np < 0 || ns < 0 || ng + np + ns + 3 > 64) return SGC_ERR_ARG;
    if (!out || !counts || (target && !norm)) return SGC_ERR_ARG;
    if (M > 0 && (!part || !cnt_part || !subject_cat || !object_cat || !aligned || !violated)) return SGC_ERR_ARG;
    if ((dir == nullptr) != (flags == nullptr)) return SGC_ERR_ARG;
    if (target) {
        SGC_LAUNCH(head_loss_norm_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, target, target_is_int64, class_weight, M, ng, np,
                   ns, norm);
        SGC_CHECK_LAUNCH();
    }
    int n_part = 0;
    if (M > 0) {
        AnyFwdParams p{};
        p.h = h; p.W = W; p.b = bias; p.M = M; p.D = D; p.ng = ng; p.np = np; p.ns = ns; p.T1 = T1; p.T2 = T2; p.T3 = T3;
        p.target = target; p.tgt64 = target_is_int64; p.cw = class_weight; p.norm = norm; p.dz = target ? dz : nullptr;
        p.scat = subject_cat; p.ocat = object_cat; p.cat64 = cat_is_int64; p.aligned = aligned; p.violated = violated; p.C = C;
        p.dir = dir; p.flags = flags;
        n_part = (M + any_fwd_tile(M) - 1) / any_fwd_tile(M);      // one partial per workgroup; at most ceil(M / 32)
        p.loss_part = part; p.cs_part = part + n_part; p.cs_cnt = cnt_part;
        const int rc = launch_any_fwd<EPI_LOSS_CS>(p, (hipStream_t)stream);
        if (rc != SGC_OK) return rc;
    }
    SGC_LAUNCH(head_cs_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, part + n_part, cnt_part, n_part, lambda_cs,
               lambda_weak, lambda_strong, out, counts);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

int sgc_bayes_head_any_loss_cs_bwd(const float* h, const float* W, const float* dz, const float* dir, const unsigned char* flags,
                                   const float* coef, const float* g, int M, int D, int ng, int np, int ns, float* dh, float* part,
                                   void* stream) {
    if (D < 1 || M < 0 || ng < 0 || np < 0 || ns < 0 || ng + np + ns + 3 > 64) return SGC_ERR_ARG;
    if (M == 0 || (!dh && !part)) return SGC_OK;
    if (!dir || !flags || !coef || !g) return SGC_ERR_ARG;
    AnyBwdParams p{};
    p.h = h; p.W = W; p.M = M; p.D = D; p.ng = ng; p.np = np; p.ns = ns; p.dh = dh; p.part = part; p.dz = dz; p.g = g;
    p.dir = dir; p.flags = flags; p.coef = coef;
    const int nx = (M + ANY_BWD_ROWS - 1) / ANY_BWD_ROWS;
    const int nquad = (D + 32 * ANY_WAVES - 1) / (32 * ANY_WAVES);
    int ny = (512 + nx - 1) / nx;
    if (ny > nquad) ny = nquad;
    const int lds = ANY_BWD_ROWS * DZ_LD * 4;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(head_any_bwd_kernel<FROM_DZ_CS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              lds);
    SGC_LAUNCH(head_any_bwd_kernel<FROM_DZ_CS>, dim3(nx, ny), dim3(256), lds, (hipStream_t)stream, p);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

int sgc_bayes_head_any_bwd(const float* h, const float* W, const float* rel, const float* sup, const float* g_rel, const float* g_sup,
                           int M, int D, int ng, int np, int ns, float T1, float T2, float T3, float* dh, float* part, void* stream) {
    if (D < 1 || M < 0 || ng < 0 || np < 0 || ns < 0 || ng + np + ns + 3 > 64) return SGC_ERR_ARG;
    if (M == 0 || (!dh && !part)) return SGC_OK;
    AnyBwdParams p{};
    p.h = h; p.W = W; p.rel = rel; p.sup = sup; p.g_rel = g_rel; p.g_sup = g_sup; p.M = M; p.D = D; p.ng = ng; p.np = np; p.ns = ns;
    p.T1 = T1; p.T2 = T2; p.T3 = T3; p.dh = dh; p.part = part;
    const int nx = (M + ANY_BWD_ROWS - 1) / ANY_BWD_ROWS;
    const int nquad = (D + 32 * ANY_WAVES - 1) / (32 * ANY_WAVES);       // 128-column groups of D
    int ny = (512 + nx - 1) / nx;                                         // about two workgroups per CU
    if (ny > nquad) ny = nquad;
    const int lds = ANY_BWD_ROWS * DZ_LD * 4;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(head_any_bwd_kernel<FROM_OUTPUTS>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    SGC_LAUNCH(head_any_bwd_kernel<FROM_OUTPUTS>, dim3(nx, ny), dim3(256), lds, (hipStream_t)stream, p);
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
