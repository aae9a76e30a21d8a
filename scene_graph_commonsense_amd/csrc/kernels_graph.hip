// Scene-graph inference: the ranked top-K (subject, predicate, object) triples of every image from ONE kernel that reads the
// forward's outputs in place (reference evaluator.py:125-134,160-194 candidate confidences and filters, :292-316 ranking,
// :465-503 the ranked edge list).  The evaluator route to the same lists appends int64 copies of every candidate to the
// Evaluator's state, permutes them into append order, filters them and then groups and ranks them (csrc/kernels_eval.hip).
#include "common.h"
#include "eval_geom.h"
#include "rank_select.h"

struct GraphParams {
    const float* cand_conf; const int* cand_pred; int rep;            // [P][rep] per-pair candidates of the head (rep = 1 or 3)
    const float* cat_conf;                                            // [P] subject + object category confidence (SGDET) or NULL
    const float* conn;                                                // [P] log-sigmoid connectivity
    const unsigned char* mask;                                        // [P] overlap filter (0 -> -inf) or NULL
    const unsigned char* included;                                    // [P] 0 = the pair is no candidate at all, or NULL
    const int* ptr; const int* list;                                  // [B+1], [ptr[B]] pair rows of every image, ascending; list NULL = identity
    const int* sub_idx; const int* obj_idx; const long* cats;         // [P], [P], [n_obj]; NULL -> subject / object come back -1
    const unsigned* aligned; const unsigned* violated; int C, R;      // commonsense bitmaps (triplet_bits' layout) or NULL
    int slot_major, K;
    int* out_pair; int* out_slot; int* out_pred; int* out_sub; int* out_obj; float* out_score;      // [B][K]
    int* out_count; int* out_finite;                                  // [B]
};

enum { GRAPH_THREADS = 1024, GRAPH_CACHE = 12288 };     // 48 KiB of cached keys: 64 objects x rep 3

// ascending uint order == ascending float order; every NaN ranks first (as torch.sort puts it); 0 is below -inf and marks a
// slot that is no candidate
__device__ __forceinline__ unsigned graph_key(float f) { return f != f ? 0xffffffffu : order_key(f); }

// local slot j of an image with m listed pairs -> (position in its list, super-category slot).  The tie order IS the order of j.
__device__ __forceinline__ void graph_decode(const GraphParams& g, int j, int m, int& i, int& s) {
    if (g.slot_major) { s = j / m; i = j - s * m; } else { i = j / g.rep; s = j - i * g.rep; }
}

// (cand_conf + cat_conf) + conn in that f32 order, -inf where the overlap mask or the commonsense sets reject the candidate
// (evaluator.py:129-134,189-194 and `confidence += connectivity` of :292)
__device__ __forceinline__ float graph_score(const GraphParams& g, int p, int s, bool& valid) {
    valid = !(g.included && g.included[p] == 0);
    if (!valid) return -INFINITY;
    float c = g.cand_conf[(long)p * g.rep + s];
    if (g.cat_conf) c = c + g.cat_conf[p];
    bool keep = !(g.mask && g.mask[p] == 0);
    if (keep && g.aligned) {
        const long sc = g.cats[g.sub_idx[p]], oc = g.cats[g.obj_idx[p]], r = g.cand_pred[(long)p * g.rep + s];
        keep = triplet_bits(g.aligned, g.violated, sc, r, oc, g.C, g.R) == 1u;      // aligned and not violated
    }
    if (!keep) c = -INFINITY;
    return c + g.conn[p];
}

__device__ __forceinline__ unsigned graph_slot_key(const GraphParams& g, int b0, int m, int j) {
    int i, s;
    graph_decode(g, j, m, i, s);
    const int p = g.list ? g.list[b0 + i] : b0 + i;
    bool valid;
    const float c = graph_score(g, p, s, valid);
    return valid ? graph_key(c) : 0u;
}

// One workgroup per image: the keys of the image's slots are formed once and kept in LDS (slots past GRAPH_CACHE are formed again
// every time the selection asks for them), then block_topk (csrc/rank_select.h) ranks them by (confidence desc, slot asc).
// Tie order = the reference's append order.  Pair-major (pair, slot) is right for fused scenes: a direction-step holds at most
// one pair of an image, so the step's blocked [geo | poss | sem] append order and the pair-major order coincide PER IMAGE.
// Slot-major (slot, pair) is right for one head.candidates call appended with call_sizes = [M].
__global__ __launch_bounds__(GRAPH_THREADS) void scene_graph_topk_kernel(const GraphParams g) {
    __shared__ unsigned cache[GRAPH_CACHE];
    __shared__ TopkScratch<GRAPH_THREADS> sel;
    __shared__ int s_valid, s_finite;
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, K = g.K;
    const int b0 = g.ptr[img], m = g.ptr[img + 1] - b0;
    const int n = m * g.rep;
    if (tid == 0) { s_valid = 0; s_finite = 0; }
    __syncthreads();
    for (int j0 = 0; j0 < n; j0 += GRAPH_THREADS) {
        const int j = j0 + tid;
        unsigned key = 0;
        if (j < n) {
            key = graph_slot_key(g, b0, m, j);
            if (j < GRAPH_CACHE) cache[j] = key;
        }
        const unsigned long long bal = __ballot(key != 0);
        if (lane == 0 && bal) atomicAdd(&s_valid, __popcll(bal));
    }
    __syncthreads();
    // k <= candidates, so the K-th largest key belongs to a candidate: it is > 0 and a non-candidate slot is never taken
    const int k = min(K, s_valid);
    block_topk<GRAPH_THREADS>(sel, n, k, [&](int j) { return j < GRAPH_CACHE ? cache[j] : graph_slot_key(g, b0, m, j); });
    // epilogue: the ranked edges (evaluator.py:482-503 reads the same fields of the ranked candidates); K <= 128 < GRAPH_THREADS
    bool finite = false;
    if (tid < K) {
        const long o = (long)img * K + tid;
        int pair = -1, slot = -1, pred = -1, sub = -1, obj = -1;
        float score = -INFINITY;
        if (tid < k) {
            const int j = (int)(sel.keys[tid] & 0xffffffffull);
            int i;
            graph_decode(g, j, m, i, slot);
            pair = g.list ? g.list[b0 + i] : b0 + i;
            bool valid;
            score = graph_score(g, pair, slot, valid);
            pred = g.cand_pred[(long)pair * g.rep + slot];
            if (g.sub_idx) sub = g.sub_idx[pair];
            if (g.obj_idx) obj = g.obj_idx[pair];
            finite = fabsf(score) <= 3.402823466e+38f;
        }
        g.out_pair[o] = pair; g.out_slot[o] = slot; g.out_pred[o] = pred; g.out_sub[o] = sub; g.out_obj[o] = obj;
        g.out_score[o] = score;
    }
    const unsigned long long fb = __ballot(finite);
    if (lane == 0 && fb) atomicAdd(&s_finite, __popcll(fb));
    __syncthreads();
    if (tid == 0) { g.out_count[img] = k; g.out_finite[img] = s_finite; }
}

extern "C" {

int sgc_scene_graph_topk(const float* cand_conf, const int* cand_pred, int rep, const float* cat_conf, const float* conn,
                         const unsigned char* mask, const unsigned char* included, const int* image_ptr, const int* pair_list,
                         const int* sub_idx, const int* obj_idx, const long* cats, const unsigned* aligned, const unsigned* violated,
                         int C, int R, int n_img, int K, int slot_major, int* out_pair, int* out_slot, int* out_pred, int* out_sub,
                         int* out_obj, float* out_score, int* out_count, int* out_finite, void* stream) {
    if (K < 1 || K > 128 || (rep != 1 && rep != 3)) return SGC_ERR_ARG;
    if ((aligned == nullptr) != (violated == nullptr)) return SGC_ERR_ARG;
    if (aligned && (!sub_idx || !obj_idx || !cats || C < 1 || R < 1)) return SGC_ERR_ARG;
    if (n_img <= 0) return SGC_OK;
    // (cand_conf / cand_pred / conn may be NULL when there is no pair at all: no image then lists a row)
    if (!image_ptr || !out_pair || !out_slot || !out_pred || !out_sub || !out_obj || !out_score || !out_count || !out_finite)
        return SGC_ERR_ARG;
    GraphParams g{cand_conf, cand_pred, rep, cat_conf, conn, mask, included, image_ptr, pair_list, sub_idx, obj_idx, cats, aligned, violated,
                  C, R, slot_major ? 1 : 0, K, out_pair, out_slot, out_pred, out_sub, out_obj, out_score, out_count, out_finite};
    SGC_LAUNCH(scene_graph_topk_kernel, dim3(n_img), dim3(GRAPH_THREADS), 0, (hipStream_t)stream, g);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

}  // extern "C"
