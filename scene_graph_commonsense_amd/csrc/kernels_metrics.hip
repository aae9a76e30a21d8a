// Device-resident evaluation metrics: the counters of Recall@K / mR@K / zero-shot recall (reference evaluator.py:306-367), of the
// Top-3 variant (:720-773) and of the OpenImages weighted mean AP (:522-566) updated straight from the ranked lists that
// sgc_scene_graph_topk writes (csrc/kernels_graph.hip) and the scene's own tables.  Nothing is compacted, copied per candidate or
// read back: a target is a pair row with directed != -1 in a kept step, a candidate's labels and boxes are cats / boxes of its
// ranked subject and object.  The counters are 64-bit integers updated with atomicAdd, so their sums do not depend on the order
// in which the wavefronts arrive.
#include "common.h"
#include "eval_geom.h"

enum { METRIC_MAX_KS = 8 };

struct RecallAccParams {
    const int* out_pair; const int* out_pred; const int* out_sub; const int* out_obj;      // [n_img][K] ranked lists
    const int* out_count; int K, n_img;                                                    // [n_img]
    const int* cand_pred; int n_pred;                       // Top-3: the head's [P][3] predicates, read through out_pair; n_pred = 1 or 3
    const long* cats; const float* boxes; int n_obj;        // per-object tables: classes, raw boxes [n_obj][4] (x0,x1,y0,y1)
    const int* sub_idx; const int* obj_idx; const int* image; const int* directed;         // [P]
    const unsigned char* included; int P;                   // [P] kept steps or NULL
    const int* img_targets;                                 // [n_img] connected targets of the kept steps per image (Top-3)
    int ks[METRIC_MAX_KS]; int n_k;
    const unsigned* zs; int C, R;                           // zero-shot bitmap (triplet_bit's layout) or NULL
    int F; double iou_thresh;
    unsigned long long* hits; unsigned long long* hits_pc; unsigned long long* tgt; unsigned long long* tgt_pc;              // [n_k], [n_k][R], [1], [R]
    unsigned long long* zs_hits; unsigned long long* zs_hits_pc; unsigned long long* zs_tgt; unsigned long long* zs_tgt_pc;  // the zero-shot twins
};

// One wavefront per pair row; rows that are no connected target of a kept step leave at once.  The scan is first_match_rank
// (csrc/eval_geom.h) with recall_hits_kernel's test: labels, both grid IoUs and the predicate must match; a candidate whose labels
// and boxes match but whose predicate differs does not end the scan; -inf candidates take part.
__global__ __launch_bounds__(256) void recall_accumulate_kernel(const RecallAccParams p) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.P) return;
    const int rel = p.directed[row];
    if (rel == -1 || (p.included && p.included[row] == 0)) return;
    const int img = p.image[row], ts = p.sub_idx[row], to = p.obj_idx[row];
    if (img < 0 || img >= p.n_img || ts < 0 || ts >= p.n_obj || to < 0 || to >= p.n_obj) return;
    const long sc = p.cats[ts], oc = p.cats[to];
    const GridBox tsb = load_box(p.boxes, ts, p.F), tob = load_box(p.boxes, to, p.F);
    const int cnt = min(p.out_count[img], p.K);
    const int hit = first_match_rank(cnt, p.K, [&](int j) {
        const long o = (long)img * p.K + j;
        const int cs = p.out_sub[o], co = p.out_obj[o];
        if (!(cs >= 0 && cs < p.n_obj && co >= 0 && co < p.n_obj && p.cats[cs] == sc && p.cats[co] == oc)) return false;
        bool pred = false;
        if (p.n_pred == 1) {
            pred = p.out_pred[o] == rel;
        } else {
            const int pr = p.out_pair[o];
            if (pr >= 0 && pr < p.P)
                for (int k = 0; k < 3; ++k) pred |= p.cand_pred[3L * pr + k] == rel;
        }
        return pred && box_iou_ok(tsb, load_box(p.boxes, cs, p.F), p.iou_thresh) &&
               box_iou_ok(tob, load_box(p.boxes, co, p.F), p.iou_thresh);
    });
    if (lane != 0) return;
    const bool cls = rel >= 0 && rel < p.R;
    const bool zs = p.zs && triplet_bit(p.zs, sc, rel, oc, p.C, p.R);
    const int n_t = p.n_pred == 3 ? p.img_targets[img] : 0;
    for (int i = 0; i < p.n_k; ++i) {
        // evaluator.py:435 `hit < k and hit < count`; Top-3 :668 `hit < count and hit < max(k, targets of the image)`
        const int bound = p.n_pred == 3 ? max(p.ks[i], n_t) : p.ks[i];
        if (hit < cnt && hit < bound) {
            atomicAdd(p.hits + i, 1ull);
            if (cls) atomicAdd(p.hits_pc + (long)i * p.R + rel, 1ull);
            if (zs) { atomicAdd(p.zs_hits + i, 1ull); atomicAdd(p.zs_hits_pc + (long)i * p.R + rel, 1ull); }
        }
    }
    atomicAdd(p.tgt, 1ull);
    if (cls) atomicAdd(p.tgt_pc + rel, 1ull);
    if (zs) { atomicAdd(p.zs_tgt, 1ull); atomicAdd(p.zs_tgt_pc + rel, 1ull); }
}

struct PrecisionAccParams {
    const int* out_pred; const int* out_sub; const int* out_obj; const int* out_count; int K, n_img, n_rank;
    const int* ptr; const int* list;                        // [n_img+1], pair rows of every image (list NULL = the rows ptr[b] .. ptr[b+1]-1)
    const long* cats; const float* boxes; int n_obj;
    const int* sub_idx; const int* obj_idx; const int* directed; const unsigned char* included; int P;
    int R, F; double iou_thresh;
    unsigned long long* ap; unsigned long long* ap_union; unsigned long long* num_ap;      // [R] each
};

// One wavefront per (image, rank j < min(n_rank, count)): lanes walk the image's pair rows 64 at a time and keep the connected
// targets of the kept steps; `found` / `found_union` are np.any over them (evaluator.py:534-557).
__global__ __launch_bounds__(256) void precision_accumulate_kernel(const PrecisionAccParams p) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int img = w / p.n_rank, j = w - img * p.n_rank;
    if (img >= p.n_img || j >= min(p.out_count[img], p.K)) return;
    const long o = (long)img * p.K + j;
    const int pj = p.out_pred[o], cs = p.out_sub[o], co = p.out_obj[o];
    if (cs < 0 || cs >= p.n_obj || co < 0 || co >= p.n_obj) return;
    const long sc = p.cats[cs], oc = p.cats[co];
    const GridBox sb = load_box(p.boxes, cs, p.F), ob = load_box(p.boxes, co, p.F);
    const int b0 = p.ptr[img], m = p.ptr[img + 1] - b0;
    bool found = false, found_union = false;
    for (int i0 = 0; i0 < m; i0 += 64) {
        const int i = i0 + lane;
        if (i >= m) continue;
        const int row = p.list ? p.list[b0 + i] : b0 + i;
        if (row < 0 || row >= p.P) continue;
        const int rel = p.directed[row];
        if (rel == -1 || rel != pj || (p.included && p.included[row] == 0)) continue;
        const int ts = p.sub_idx[row], to = p.obj_idx[row];
        if (ts < 0 || ts >= p.n_obj || to < 0 || to >= p.n_obj || p.cats[ts] != sc || p.cats[to] != oc) continue;
        const GridBox tsb = load_box(p.boxes, ts, p.F), tob = load_box(p.boxes, to, p.F);
        found |= box_iou_ok(tsb, sb, p.iou_thresh) && box_iou_ok(tob, ob, p.iou_thresh);
        found_union |= union_iou_ok(sb, ob, tsb, tob, p.iou_thresh);
    }
    const bool any_found = __ballot(found) != 0, any_union = __ballot(found_union) != 0;
    if (lane != 0 || pj < 0 || pj >= p.R) return;
    atomicAdd(p.num_ap + pj, 1ull);
    if (any_found) atomicAdd(p.ap + pj, 1ull);
    if (any_union) atomicAdd(p.ap_union + pj, 1ull);
}

extern "C" {

int sgc_recall_accumulate(const int* out_pair, const int* out_pred, const int* out_sub, const int* out_obj, const int* out_count,
                          int n_img, int K, const int* cand_pred, int n_pred, const long* cats, const float* boxes, int n_obj,
                          const int* sub_idx, const int* obj_idx, const int* image, const int* directed,
                          const unsigned char* included, int n_pairs, const int* img_targets, const int* top_k, int n_k,
                          const unsigned* zero_shot, int C, int R, int feature_size, double iou_thresh, long* hits, long* hits_pc,
                          long* targets, long* targets_pc, long* zs_hits, long* zs_hits_pc, long* zs_targets, long* zs_targets_pc,
                          void* stream) {
    if (K < 1 || K > 128 || (n_pred != 1 && n_pred != 3) || n_k < 1 || n_k > METRIC_MAX_KS || !top_k || R < 1) return SGC_ERR_ARG;
    if (n_pred == 3 && (!cand_pred || !img_targets || !out_pair)) return SGC_ERR_ARG;
    if (zero_shot && (C < 1 || !zs_hits || !zs_hits_pc || !zs_targets || !zs_targets_pc)) return SGC_ERR_ARG;
    if (n_pairs <= 0 || n_img <= 0) return SGC_OK;
    if (!out_pred || !out_sub || !out_obj || !out_count || !cats || !boxes || !sub_idx || !obj_idx || !image || !directed || !hits ||
        !hits_pc || !targets || !targets_pc)
        return SGC_ERR_ARG;
    typedef unsigned long long u64;
    RecallAccParams p{out_pair, out_pred, out_sub, out_obj, out_count, K, n_img, cand_pred, n_pred, cats, boxes, n_obj, sub_idx, obj_idx,
                      image, directed, included, n_pairs, img_targets, {0}, n_k, zero_shot, C, R, feature_size, iou_thresh,
                      (u64*)hits, (u64*)hits_pc, (u64*)targets, (u64*)targets_pc, (u64*)zs_hits, (u64*)zs_hits_pc, (u64*)zs_targets,
                      (u64*)zs_targets_pc};
    for (int i = 0; i < n_k; ++i) p.ks[i] = top_k[i];                  // top_k is a HOST array
    SGC_LAUNCH(recall_accumulate_kernel, dim3((n_pairs + 3) / 4), dim3(256), 0, (hipStream_t)stream, p);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

int sgc_precision_accumulate(const int* out_pred, const int* out_sub, const int* out_obj, const int* out_count, int n_img, int K,
                             int n_rank, const int* image_ptr, const int* pair_list, const long* cats, const float* boxes, int n_obj,
                             const int* sub_idx, const int* obj_idx, const int* directed, const unsigned char* included, int n_pairs,
                             int R, int feature_size, double iou_thresh, long* ap, long* ap_union, long* num_ap, void* stream) {
    if (K < 1 || K > 128 || n_rank < 1 || n_rank > K || R < 1) return SGC_ERR_ARG;
    if (n_img <= 0) return SGC_OK;
    if (!out_pred || !out_sub || !out_obj || !out_count || !image_ptr || !cats || !boxes || !sub_idx || !obj_idx || !directed || !ap ||
        !ap_union || !num_ap)
        return SGC_ERR_ARG;
    typedef unsigned long long u64;
    PrecisionAccParams p{out_pred, out_sub, out_obj, out_count, K, n_img, n_rank, image_ptr, pair_list, cats, boxes, n_obj, sub_idx,
                         obj_idx, directed, included, n_pairs, R, feature_size, iou_thresh, (u64*)ap, (u64*)ap_union, (u64*)num_ap};
    const long waves = (long)n_img * n_rank;
    SGC_LAUNCH(precision_accumulate_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

}  // extern "C"
