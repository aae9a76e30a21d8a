// Device-resident evaluation metrics: the counters of Recall@K / mR@K / zero-shot recall (reference evaluator.py:306-367), of the
// Top-3 variant (:720-773) and of the OpenImages weighted mean AP (:522-566) updated straight from the ranked lists that
// sgc_scene_graph_topk writes (csrc/kernels_graph.hip) and the scene's own tables.  Nothing is compacted, copied per candidate or
// read back: a target is a pair row with directed != -1 in a kept step, a candidate's labels and boxes are cats / boxes of its
// ranked subject and object.  The counters are 64-bit integers updated with atomicAdd, so their sums do not depend on the order
// in which the wavefronts arrive.
#include "common.h"
#include "eval_geom.h"

enum { METRIC_MAX_KS = 8 };

typedef unsigned long long u64;

// The eight counter arrays of one Recall@K family and what decides their update, shared by the two accumulate kernels.
struct RecallCounters {
    int ks[METRIC_MAX_KS]; int n_k;
    const unsigned* zs; int C, R;                           // zero-shot bitmap (triplet_bit's layout) or NULL
    u64* hits; u64* hits_pc; u64* tgt; u64* tgt_pc;                  // [n_k], [n_k][R], [1], [R]
    u64* zs_hits; u64* zs_hits_pc; u64* zs_tgt; u64* zs_tgt_pc;      // the zero-shot twins
};

// One target with classes (sc, oc), predicate rel and first matching rank `hit` among the cnt ranked candidates of its image
// (evaluator.py:336-356).  One lane calls this.  top3_targets >= 0: the Top-3 bound max(k, targets of the image); -1: k.
__device__ __forceinline__ void count_target(const RecallCounters& c, long sc, long rel, long oc, int hit, int cnt, int top3_targets) {
    const bool cls = rel >= 0 && rel < c.R;
    const bool zs = c.zs && triplet_bit(c.zs, sc, rel, oc, c.C, c.R);
    for (int i = 0; i < c.n_k; ++i) {
        // evaluator.py:435 `hit < k and hit < count`; Top-3 :668 `hit < count and hit < max(k, targets of the image)`
        const int bound = top3_targets >= 0 ? max(c.ks[i], top3_targets) : c.ks[i];
        if (hit < cnt && hit < bound) {
            atomicAdd(c.hits + i, 1ull);
            if (cls) atomicAdd(c.hits_pc + (long)i * c.R + rel, 1ull);
            if (zs) { atomicAdd(c.zs_hits + i, 1ull); atomicAdd(c.zs_hits_pc + (long)i * c.R + rel, 1ull); }
        }
    }
    atomicAdd(c.tgt, 1ull);
    if (cls) atomicAdd(c.tgt_pc + rel, 1ull);
    if (zs) { atomicAdd(c.zs_tgt, 1ull); atomicAdd(c.zs_tgt_pc + rel, 1ull); }
}

struct RecallAccParams {
    const int* out_pair; const int* out_pred; const int* out_sub; const int* out_obj;      // [n_img][K] ranked lists
    const int* out_count; int K, n_img;                                                    // [n_img]
    const int* cand_pred; int n_pred;                       // Top-3: the head's [P][3] predicates, read through out_pair; n_pred = 1 or 3
    const long* cats; const float* boxes; int n_obj;        // per-object tables: classes, raw boxes [n_obj][4] (x0,x1,y0,y1)
    const int* sub_idx; const int* obj_idx; const int* image; const int* directed;         // [P]
    const unsigned char* included; int P;                   // [P] kept steps or NULL
    const int* img_targets;                                 // [n_img] connected targets of the kept steps per image (Top-3)
    int F; double iou_thresh;
    RecallCounters c;
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
    if (lane == 0) count_target(p.c, sc, rel, oc, hit, cnt, p.n_pred == 3 ? p.img_targets[img] : -1);
}

// SGDET / SGCLS (evaluator.py:272-277, 306-356 with predcls=False): the targets are ground-truth triples of their own - image,
// predicate, classes and boxes per row of a target table (pairs.sg_target_table) - and the candidates are the ranked pairs of the
// PREDICTED objects; labels match by equality or through the reference's equivalence classes (utils.py:355-373, `equiv`
// [n_equiv][n_equiv] u8 or NULL).  The target table's box rows carry no alignment promise (four-load load_box); `boxes` is the
// scene's 16-byte aligned table.
struct RecallTgtParams {
    const int* out_pred; const int* out_sub; const int* out_obj; const int* out_count; int K, n_img;
    const long* cats; const float* boxes; int n_obj;
    const int* t_image; const long* t_rel; const long* t_scat; const long* t_ocat; const float* t_sbox; const float* t_obox; int n_t;
    const unsigned char* equiv; int n_equiv;
    int F; double iou_thresh;
    RecallCounters c;
};

// One wavefront per row of the target table.  A row with predicate -1, with an image out of range or with an image that owns no
// candidate leaves at once and is not counted as a target: Evaluator.compute visits the images of the candidates only.  The scan
// and the test are recall_hits_kernel's with one predicate per candidate.
__global__ __launch_bounds__(256) void recall_accumulate_targets_kernel(const RecallTgtParams p) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= p.n_t) return;
    const long rel = p.t_rel[t];
    const int img = p.t_image[t];
    if (rel == -1 || img < 0 || img >= p.n_img) return;
    const int cnt = min(p.out_count[img], p.K);
    if (cnt <= 0) return;
    const long sc = p.t_scat[t], oc = p.t_ocat[t];
    const GridBox tsb = load_box(p.t_sbox + 4L * t, p.F), tob = load_box(p.t_obox + 4L * t, p.F);
    const bool t_in = sc >= 0 && sc < p.n_equiv && oc >= 0 && oc < p.n_equiv;
    const int hit = first_match_rank(cnt, p.K, [&](int j) {
        const long o = (long)img * p.K + j;
        const int cs = p.out_sub[o], co = p.out_obj[o];
        if (!(cs >= 0 && cs < p.n_obj && co >= 0 && co < p.n_obj)) return false;
        const long csc = p.cats[cs], coc = p.cats[co];
        bool label = csc == sc && coc == oc;
        if (p.equiv && !label) {
            const bool in = t_in && csc >= 0 && csc < p.n_equiv && coc >= 0 && coc < p.n_equiv;
            label = in && p.equiv[sc * p.n_equiv + csc] && p.equiv[oc * p.n_equiv + coc];
        }
        return label && p.out_pred[o] == rel && box_iou_ok(tsb, load_box(p.boxes, cs, p.F), p.iou_thresh) &&
               box_iou_ok(tob, load_box(p.boxes, co, p.F), p.iou_thresh);
    });
    if (lane == 0) count_target(p.c, sc, rel, oc, hit, cnt, -1);
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
    RecallAccParams p{out_pair, out_pred, out_sub, out_obj, out_count, K, n_img, cand_pred, n_pred, cats, boxes, n_obj, sub_idx, obj_idx,
                      image, directed, included, n_pairs, img_targets, feature_size, iou_thresh,
                      {{0}, n_k, zero_shot, C, R, (u64*)hits, (u64*)hits_pc, (u64*)targets, (u64*)targets_pc, (u64*)zs_hits,
                       (u64*)zs_hits_pc, (u64*)zs_targets, (u64*)zs_targets_pc}};
    for (int i = 0; i < n_k; ++i) p.c.ks[i] = top_k[i];                // top_k is a HOST array
    SGC_LAUNCH(recall_accumulate_kernel, dim3((n_pairs + 3) / 4), dim3(256), 0, (hipStream_t)stream, p);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

int sgc_recall_accumulate_targets(const int* out_pred, const int* out_sub, const int* out_obj, const int* out_count, int n_img, int K,
                                  const long* cats, const float* boxes, int n_obj, const int* t_image, const long* t_rel,
                                  const long* t_scat, const long* t_ocat, const float* t_sbox, const float* t_obox, int n_targets,
                                  const unsigned char* equiv, int n_equiv, const int* top_k, int n_k, const unsigned* zero_shot, int C,
                                  int R, int feature_size, double iou_thresh, long* hits, long* hits_pc, long* targets,
                                  long* targets_pc, long* zs_hits, long* zs_hits_pc, long* zs_targets, long* zs_targets_pc,
                                  void* stream) {
    if (K < 1 || K > 128 || n_k < 1 || n_k > METRIC_MAX_KS || !top_k || R < 1 || (equiv && n_equiv < 1)) return SGC_ERR_ARG;
    if (zero_shot && (C < 1 || !zs_hits || !zs_hits_pc || !zs_targets || !zs_targets_pc)) return SGC_ERR_ARG;
    if (n_targets <= 0 || n_img <= 0) return SGC_OK;
    if (!out_pred || !out_sub || !out_obj || !out_count || !cats || !boxes || !t_image || !t_rel || !t_scat || !t_ocat || !t_sbox ||
        !t_obox || !hits || !hits_pc || !targets || !targets_pc)
        return SGC_ERR_ARG;
    RecallTgtParams p{out_pred, out_sub, out_obj, out_count, K, n_img, cats, boxes, n_obj, t_image, t_rel, t_scat, t_ocat, t_sbox, t_obox,
                      n_targets, equiv, equiv ? n_equiv : 0, feature_size, iou_thresh,
                      {{0}, n_k, zero_shot, C, R, (u64*)hits, (u64*)hits_pc, (u64*)targets, (u64*)targets_pc, (u64*)zs_hits,
                       (u64*)zs_hits_pc, (u64*)zs_targets, (u64*)zs_targets_pc}};
    for (int i = 0; i < n_k; ++i) p.c.ks[i] = top_k[i];                // top_k is a HOST array
    SGC_LAUNCH(recall_accumulate_targets_kernel, dim3((n_targets + 3) / 4), dim3(256), 0, (hipStream_t)stream, p);
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
    PrecisionAccParams p{out_pred, out_sub, out_obj, out_count, K, n_img, n_rank, image_ptr, pair_list, cats, boxes, n_obj, sub_idx,
                         obj_idx, directed, included, n_pairs, R, feature_size, iou_thresh, (u64*)ap, (u64*)ap_union, (u64*)num_ap};
    const long waves = (long)n_img * n_rank;
    SGC_LAUNCH(precision_accumulate_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

}  // extern "C"
