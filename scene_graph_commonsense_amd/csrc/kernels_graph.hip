// Scene-graph inference: the ranked top-K (subject, predicate, object) triples of every image from ONE kernel that reads the
// forward's outputs in place (reference evaluator.py:125-134,160-194 candidate confidences and filters, :292-316 ranking,
// :465-503 the ranked edge list).  The evaluator route to the same lists appends int64 copies of every candidate to the
// Evaluator's state, permutes them into append order, filters them and then groups and ranks them (csrc/kernels_eval.hip).
#include "common.h"

struct GraphParams {
    const float* cand_conf; const int* cand_pred; int rep;            // [P][rep] per-pair candidates of the head (rep = 1 or 3)
    const float* cat_conf;                                            // [P] subject + object category confidence (SGDET) or NULL
    const float* conn;                                                // [P] log-sigmoid connectivity
    const unsigned char* mask;                                        // [P] overlap filter (0 -> -inf) or NULL
    const unsigned char* included;                                    // [P] 0 = the pair is no candidate at all, or NULL
    const int* ptr; const int* list;                                  // [B+1], [ptr[B]] pair rows of every image, ascending; list NULL = identity
    const int* sub_idx; const int* obj_idx; const long* cats;         // [P], [P], [n_obj]; NULL -> subject / object come back -1
    const unsigned* aligned; const unsigned* violated; int C, R;      // commonsense bitmaps (sgc_commonsense_filter's layout) or NULL
    int slot_major, K;
    int* out_pair; int* out_slot; int* out_pred; int* out_sub; int* out_obj; float* out_score;      // [B][K]
    int* out_count; int* out_finite;                                  // [B]
};

enum { GRAPH_THREADS = 1024, GRAPH_WAVES = GRAPH_THREADS / 64, GRAPH_CACHE = 12288 };     // 48 KiB of cached keys: 64 objects x rep 3

// ascending uint order == ascending float order; every NaN ranks first (as torch.sort puts it); 0 is below -inf and marks a
// slot that is no candidate
__device__ __forceinline__ unsigned graph_key(float f) {
    if (f != f) return 0xffffffffu;
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

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
        keep = false;
        if (sc >= 0 && sc < g.C && oc >= 0 && oc < g.C && r >= 0 && r < g.R) {
            const long bit = (sc * g.R + r) * g.C + oc;
            const bool in_yes = (g.aligned[bit >> 5] >> (bit & 31)) & 1u;
            const bool in_no = (g.violated[bit >> 5] >> (bit & 31)) & 1u;
            keep = in_yes && !in_no;
        }
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

// One workgroup per image, the selection scheme of topk_kernel (csrc/kernels_eval.hip): the keys of the image's slots are formed
// once and kept in LDS (slots past GRAPH_CACHE are formed again in every pass), radix-select of the K-th largest, everything above
// it plus the earliest ties by ordered compaction, bitonic sort of the <= 128 survivors by (confidence desc, slot asc).
// Tie order = the reference's append order.  Pair-major (pair, slot) is right for fused scenes: a direction-step holds at most
// one pair of an image, so the step's blocked [geo | poss | sem] append order and the pair-major order coincide PER IMAGE.
// Slot-major (slot, pair) is right for one head.candidates call appended with call_sizes = [M].
__global__ __launch_bounds__(GRAPH_THREADS) void scene_graph_topk_kernel(const GraphParams g) {
    __shared__ unsigned cache[GRAPH_CACHE];
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix, s_mask;
    __shared__ int s_remaining, s_cnt, s_base, s_valid, s_finite, wave_cnt[GRAPH_WAVES];
    __shared__ unsigned long long keys[128];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, K = g.K;
    const int b0 = g.ptr[img], m = g.ptr[img + 1] - b0;
    const int n = m * g.rep;
    if (tid < 128) keys[tid] = ~0ull;
    if (tid == 0) { s_prefix = 0; s_mask = 0; s_cnt = 0; s_valid = 0; s_finite = 0; }
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
    const int k = min(K, s_valid);
    if (tid == 0) s_remaining = k;
    __syncthreads();
#define GRAPH_KEY(j) ((j) < GRAPH_CACHE ? cache[j] : graph_slot_key(g, b0, m, (j)))
    if (k > 0) {
        for (int pass = 3; pass >= 0; --pass) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const unsigned prefix = s_prefix, mask = s_mask;
            for (int j = tid; j < n; j += GRAPH_THREADS) {
                const unsigned key = GRAPH_KEY(j);
                if ((key & mask) == prefix) atomicAdd(&hist[(key >> (8 * pass)) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                int cum = 0, rem = s_remaining;
                for (int bk = 255; bk >= 0; --bk) {
                    const int hv = (int)hist[bk];
                    if (cum + hv >= rem) {
                        s_prefix = prefix | ((unsigned)bk << (8 * pass));
                        s_mask = mask | (0xffu << (8 * pass));
                        s_remaining = rem - cum;
                        break;
                    }
                    cum += hv;
                }
            }
            __syncthreads();
        }
        // the K-th largest key belongs to a candidate (k <= candidates), so thr > 0 and a non-candidate slot is never taken;
        // fewer than k keys lie above thr, so the unordered positions stay inside keys[]
        const unsigned thr = s_prefix;
        for (int j = tid; j < n; j += GRAPH_THREADS) {
            const unsigned key = GRAPH_KEY(j);
            if (key > thr) {
                const int pos = atomicAdd(&s_cnt, 1);
                if (pos < 128) keys[pos] = ((unsigned long long)(~key) << 32) | (unsigned)j;
            }
        }
        __syncthreads();
        if (tid == 0) s_base = s_cnt;
        __syncthreads();
        for (int c0 = 0; c0 < n; c0 += GRAPH_THREADS) {
            if (s_base >= k) break;
            const int j = c0 + tid;
            const bool flag = j < n && GRAPH_KEY(j) == thr;
            const unsigned long long bal = __ballot(flag);
            const int within = __popcll(bal & ((1ull << lane) - 1ull));
            if (lane == 0) wave_cnt[wv] = __popcll(bal);
            __syncthreads();
            int off = s_base + within, total = 0;
            for (int w2 = 0; w2 < GRAPH_WAVES; ++w2) {
                if (w2 < wv) off += wave_cnt[w2];
                total += wave_cnt[w2];
            }
            if (flag && off < k) keys[off] = ((unsigned long long)(~thr) << 32) | (unsigned)j;
            __syncthreads();
            if (tid == 0) s_base += total;
            __syncthreads();
        }
        // bitonic sort of 128 keys, ascending ( = confidence descending, slot ascending)
        for (int size = 2; size <= 128; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                if (tid < 64) {
                    const int lo = 2 * tid - (tid & (stride - 1));
                    const int hi = lo + stride;
                    const bool up = ((lo & size) == 0);
                    const unsigned long long a = keys[lo], bb = keys[hi];
                    if ((a > bb) == up) { keys[lo] = bb; keys[hi] = a; }
                }
            }
        }
        __syncthreads();
    }
#undef GRAPH_KEY
    // epilogue: the ranked edges (evaluator.py:482-503 reads the same fields of the ranked candidates); K <= 128 < GRAPH_THREADS
    bool finite = false;
    if (tid < K) {
        const long o = (long)img * K + tid;
        int pair = -1, slot = -1, pred = -1, sub = -1, obj = -1;
        float score = -INFINITY;
        if (tid < k) {
            const int j = (int)(keys[tid] & 0xffffffffull);
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
