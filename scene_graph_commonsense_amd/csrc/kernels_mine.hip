// Commonsense candidate mining (run_mode prepare_cs): per image, the ranked candidates that share an endpoint with a connected
// ground-truth triple (reference evaluator.py:375-416, the body of _get_related_top_k_predictions before the LLM query).
#include "common.h"

struct RelatedParams {
    const long* c_scat; const long* c_ocat; const long* c_pred;      // candidates (flat, int64)
    const float* c_sbox; const float* c_obox; const float* c_conf;    // [n][4] (x0,x1,y0,y1), [n]
    const int* keep_pos; const int* keep_cnt;                         // [n_img][K] flat candidate positions in ranked order, [n_img]
    const int* t_ptr; const long* t_scat; const long* t_ocat;         // connected targets of image b: t_ptr[b] .. t_ptr[b+1]-1
    const float* t_sbox; const float* t_obox;
    int n_img, n_cand, K, top_k;
    int* out_pos; int* out_rank; int* out_count; float* out_conf;     // [n_img][16] x3 (-1 / -1 / NaN padded; out_conf may be NULL), [n_img]
};

// what one lane keeps of the candidate at one rank
struct RankedCand {
    long scat, ocat, pred;
    float sb[4], ob[4];
    int pos;
    bool valid;
};

__device__ __forceinline__ RankedCand load_ranked(const RelatedParams& p, int img, int j, int n_rank) {
    RankedCand c;
    c.valid = false; c.pos = -1; c.scat = c.ocat = c.pred = -1;
    for (int k = 0; k < 4; ++k) c.sb[k] = c.ob[k] = 0.f;
    if (j < n_rank) {
        const int pos = p.keep_pos[(long)img * p.K + j];
        if (pos >= 0 && pos < p.n_cand) {
            c.valid = true; c.pos = pos;
            c.scat = p.c_scat[pos]; c.ocat = p.c_ocat[pos]; c.pred = p.c_pred[pos];
            const float4 s = *reinterpret_cast<const float4*>(p.c_sbox + 4L * pos);
            const float4 o = *reinterpret_cast<const float4*>(p.c_obox + 4L * pos);
            c.sb[0] = s.x; c.sb[1] = s.y; c.sb[2] = s.z; c.sb[3] = s.w;
            c.ob[0] = o.x; c.ob[1] = o.y; c.ob[2] = o.z; c.ob[3] = o.w;
        }
    }
    return c;
}

__device__ __forceinline__ bool related(const RankedCand& c, long ts, long to, const float4& tsb, const float4& tob) {
    const bool s = c.scat == ts && c.sb[0] == tsb.x && c.sb[1] == tsb.y && c.sb[2] == tsb.z && c.sb[3] == tsb.w;
    const bool o = c.ocat == to && c.ob[0] == tob.x && c.ob[1] == tob.y && c.ob[2] == tob.z && c.ob[3] == tob.w;
    return c.valid && (s || o);
}

__device__ __forceinline__ long shfl_long(long v, int src) {
    const int lo = __shfl((int)(v & 0xffffffffL), src), hi = __shfl((int)(v >> 32), src);
    return ((long)hi << 32) | (unsigned)lo;
}

// One wavefront per image.  Lane l keeps the candidates at ranks l and l + 64 in registers; per target one compare and a ballot per
// register set give the mask of related ranks, whose set bits are then taken in ascending order.  The accepted (subject class,
// predicate, object class) keys live one per lane in lanes 0 .. 15; the duplicate test is a second ballot.  The reference's loop is
// restated literally: `count >= 10` is tested after EVERY rank, so once an image has 10 edges every later target looks at rank 0 only
// (and can still accept it: 11 edges at most); the `count >= 15` test before a target can therefore never fire and is kept as written.
__global__ __launch_bounds__(256) void related_topk_kernel(const RelatedParams p) {
    const int lane = threadIdx.x & 63;
    const int img = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (img >= p.n_img) return;                                       // whole wavefronts leave: the ballots below stay complete
    const int n_rank = min(p.top_k, min(p.keep_cnt[img], p.K));
    const RankedCand c0 = load_ranked(p, img, lane, n_rank), c1 = load_ranked(p, img, lane + 64, n_rank);
    long k_s = -1, k_p = -1, k_o = -1;                                // accepted key / output of slot `lane` (lanes 0 .. 15)
    int a_pos = -1, a_rank = -1;
    int count = 0;
    const int t0 = p.t_ptr[img], t1 = p.t_ptr[img + 1];
    for (int t = t0; t < t1; ++t) {
        if (count >= 15) break;
        const long ts = p.t_scat[t], to = p.t_ocat[t];
        const float4 tsb = *reinterpret_cast<const float4*>(p.t_sbox + 4L * t);
        const float4 tob = *reinterpret_cast<const float4*>(p.t_obox + 4L * t);
        unsigned long long m[2];
        m[0] = __ballot(related(c0, ts, to, tsb, tob));
        m[1] = p.top_k > 64 ? __ballot(related(c1, ts, to, tsb, tob)) : 0ull;
        if (count >= 10) { m[0] &= 1ull; m[1] = 0ull; }               // `if len(curr_image_graph) >= 10: break` right after rank 0
        bool full = false;                                            // the same break, reached by an accept of this target
        for (int h = 0; h < 2; ++h) {
            unsigned long long bits = m[h];
            while (bits && !full) {
                const int src = __ffsll((long long)bits) - 1;
                bits &= bits - 1;
                const long cs = shfl_long(h ? c1.scat : c0.scat, src), cp = shfl_long(h ? c1.pred : c0.pred, src),
                           co = shfl_long(h ? c1.ocat : c0.ocat, src);
                const int cpos = __shfl(h ? c1.pos : c0.pos, src);
                const bool dup = __ballot(lane < count && k_s == cs && k_p == cp && k_o == co) != 0ull;
                if (!dup && count < 16) {
                    if (lane == count) { k_s = cs; k_p = cp; k_o = co; a_pos = cpos; a_rank = h * 64 + src; }
                    ++count;
                    full = count >= 10;
                }
            }
        }
    }
    if (lane < 16) {
        const long o = (long)img * 16 + lane;
        p.out_pos[o] = a_pos;
        p.out_rank[o] = a_rank;
        if (p.out_conf) p.out_conf[o] = a_pos >= 0 ? p.c_conf[a_pos] : __uint_as_float(0x7fc00000u);
    }
    if (lane == 0) p.out_count[img] = count;
}

extern "C" {

int sgc_related_topk(const long* c_scat, const long* c_ocat, const long* c_pred, const float* c_sbox, const float* c_obox,
                     const float* c_conf, int n_cand, const int* keep_pos, const int* keep_cnt, int K, int top_k, const int* t_ptr,
                     const long* t_scat, const long* t_ocat, const float* t_sbox, const float* t_obox, int n_img, int* out_pos,
                     int* out_rank, int* out_count, float* out_conf, void* stream) {
    if (top_k < 1 || top_k > K || K > 128 || n_cand < 0) return SGC_ERR_ARG;
    if (out_conf && !c_conf) return SGC_ERR_ARG;
    if (((uintptr_t)c_sbox | (uintptr_t)c_obox | (uintptr_t)t_sbox | (uintptr_t)t_obox) & 15) return SGC_ERR_ARG;   // float4 loads
    if (n_img <= 0) return SGC_OK;
    RelatedParams p{c_scat, c_ocat, c_pred, c_sbox, c_obox, c_conf, keep_pos, keep_cnt, t_ptr, t_scat, t_ocat, t_sbox, t_obox,
                    n_img, n_cand, K, top_k, out_pos, out_rank, out_count, out_conf};
    SGC_LAUNCH(related_topk_kernel, dim3((n_img + 3) / 4), dim3(256), 0, (hipStream_t)stream, p);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

}  // extern "C"
