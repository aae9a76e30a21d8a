// Evaluation-side kernels: overlap filter (K10) and per-image stable top-K ranking (K9).
#include "common.h"
#include "eval_geom.h"
#include "rank_select.h"

// iou_mask of testing(): reference train_test.py:403-408 computes sum(mask_g | mask_e) / sum(mask_g & mask_e),
// maps inf -> 0 and keeps ratio > 0, i.e. "the two rectangles share at least one grid cell"
// (0/0 = NaN and x/0 = inf both end up False).
__global__ void overlap_filter_kernel(const int* __restrict__ bbox, const int* __restrict__ sub, const int* __restrict__ obj,
                                      unsigned char* __restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int* a = bbox + 4 * sub[i];
    const int* b = bbox + 4 * obj[i];
    const int w = min(a[1], b[1]) - max(a[0], b[0]);
    const int h = min(a[3], b[3]) - max(a[2], b[2]);
    const bool a_ok = a[1] > a[0] && a[3] > a[2], b_ok = b[1] > b[0] && b[3] > b[2];
    out[i] = (a_ok && b_ok && w > 0 && h > 0) ? 1 : 0;
}

// One workgroup per image: block_topk (csrc/rank_select.h) over the image's confidences.  Equivalent to a stable descending
// argsort truncated to K (reference evaluator.py:304,315-316 uses an unstable argsort; ties are resolved by append order here).
__global__ __launch_bounds__(256) void topk_kernel(const float* __restrict__ conf, const int* __restrict__ seg_ptr, int K,
                                                   int* __restrict__ out_idx, int* __restrict__ out_count) {
    __shared__ TopkScratch<256> sel;
    const int img = blockIdx.x, tid = threadIdx.x;
    const int b = seg_ptr[img], n = seg_ptr[img + 1] - b;
    const int k = min(K, n);
    const float* c = conf + b;
    if (tid == 0) out_count[img] = k;
    block_topk<256>(sel, n, k, [&](int i) { return order_key(c[i]); });
    for (int j = tid; j < K; j += 256) out_idx[(long)img * K + j] = (j < k) ? (int)(sel.keys[j] & 0xffffffffull) : -1;
}

// Commonsense filter of eval_cs / train_cs (reference evaluator.py:189-194,261-266): a candidate whose
// (subject class, predicate, object class) triplet is in the "violated" set or is not in the "aligned" set gets
// confidence -inf.  The Python-set membership tests become two bit lookups in C*R*C-bit device bitmaps (triplet_bit, csrc/eval_geom.h).
__global__ void commonsense_filter_kernel(const long* __restrict__ scat, const long* __restrict__ pred, const long* __restrict__ ocat,
                                          float* __restrict__ conf, int n, const unsigned* __restrict__ aligned,
                                          const unsigned* __restrict__ violated, int C, int R) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (triplet_bits(aligned, violated, scat[i], pred[i], ocat[i], C, R) != 1u) conf[i] = -INFINITY;      // keep = aligned and not violated
}

// train_cs (reference train_utils.py:36-50): per candidate (pair, super-category) flags "triplet not in the aligned set"
// (weak penalty) and "triplet in the violated set" (strong penalty).  cand_pred [n_pairs][n_cand] int32.
__global__ void commonsense_flags_kernel(const long* __restrict__ scat, const long* __restrict__ ocat, const int* __restrict__ cand_pred,
                                         int n_pairs, int n_cand, const unsigned* __restrict__ aligned,
                                         const unsigned* __restrict__ violated, int C, int R, float* __restrict__ weak,
                                         float* __restrict__ strong) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pairs * n_cand) return;
    const int pr = i / n_cand;
    const long s = scat[pr], o = ocat[pr], r = cand_pred[i];
    const unsigned in = triplet_bits(aligned, violated, s, r, o, C, R);
    weak[i] = (in & 1u) ? 0.f : 1.f;
    strong[i] = (in & 2u) ? 1.f : 0.f;
}

// Recall@K hit test (reference evaluator.py:306-356, Top-3 variant :720-760): for every connected ground-truth triple, the rank
// j of the first of its image's K ranked candidates with matching subject / object labels, both grid IoUs >= the threshold AND a
// matching predicate (a candidate whose labels and boxes match but whose predicate differs does not end the scan), or K.
// One wavefront per triple: lane l tests candidates l, l+64, ...; a ballot gives the first matching rank.
struct RecallParams {
    const long* c_scat; const long* c_ocat; const long* c_pred;      // candidates (flat); c_pred [n][n_pred]
    const float* c_sbox; const float* c_obox;                         // [n][4] (x0,x1,y0,y1) as stored (int() truncation applied here)
    const int* keep_pos; const int* keep_cnt;                         // [n_img][K] flat candidate positions in ranked order, [n_img]
    const int* t_row; const long* t_rel; const long* t_scat; const long* t_ocat; const float* t_sbox; const float* t_obox;
    const unsigned char* equiv; int n_equiv;                          // label equivalence table (SGDET/SGCLS, utils.py:355-373) or NULL
    int n_t, K, n_pred, F; double iou_thresh;
    int* hit;
};

// The box tables come from the caller with no alignment promise, so their rows are read with the four-load load_box.
__global__ __launch_bounds__(256) void recall_hits_kernel(const RecallParams p) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= p.n_t) return;
    const int row = p.t_row[t], cnt = p.keep_cnt[row];
    const long rel = p.t_rel[t], sc = p.t_scat[t], oc = p.t_ocat[t];
    const int hit = first_match_rank(cnt, p.K, [&](int j) {
        const long c = p.keep_pos[(long)row * p.K + j];
        const long cs = p.c_scat[c], co = p.c_ocat[c];
        bool label = (cs == sc) && (co == oc);
        if (p.equiv && !label) {
            const bool in = sc >= 0 && sc < p.n_equiv && oc >= 0 && oc < p.n_equiv && cs >= 0 && cs < p.n_equiv && co >= 0 && co < p.n_equiv;
            label = in && p.equiv[sc * p.n_equiv + cs] && p.equiv[oc * p.n_equiv + co];
        }
        if (!label) return false;
        bool pred = false;
        for (int k = 0; k < p.n_pred; ++k) pred |= p.c_pred[c * p.n_pred + k] == rel;
        return pred && box_iou_ok(load_box(p.t_sbox + 4L * t, p.F), load_box(p.c_sbox + 4 * c, p.F), p.iou_thresh) &&
               box_iou_ok(load_box(p.t_obox + 4L * t, p.F), load_box(p.c_obox + 4 * c, p.F), p.iou_thresh);
    });
    if ((threadIdx.x & 63) == 0) p.hit[t] = hit;
}

extern "C" {

int sgc_recall_hits(const long* c_scat, const long* c_ocat, const long* c_pred, int n_pred, const float* c_sbox, const float* c_obox,
                    const int* keep_pos, const int* keep_cnt, int K, const int* t_row, const long* t_rel, const long* t_scat,
                    const long* t_ocat, const float* t_sbox, const float* t_obox, int n_targets, const unsigned char* equiv, int n_equiv,
                    int feature_size, double iou_thresh, int* hit, void* stream) {
    if (n_targets <= 0) return SGC_OK;
    if (n_pred < 1 || K < 1) return SGC_ERR_ARG;
    RecallParams p{c_scat, c_ocat, c_pred, c_sbox, c_obox, keep_pos, keep_cnt, t_row, t_rel, t_scat, t_ocat, t_sbox, t_obox, equiv, n_equiv,
                   n_targets, K, n_pred, feature_size, iou_thresh, hit};
    SGC_LAUNCH(recall_hits_kernel, dim3((n_targets + 3) / 4), dim3(256), 0, (hipStream_t)stream, p);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

int sgc_commonsense_flags(const long* scat, const long* ocat, const int* cand_pred, int n_pairs, int n_cand, const unsigned* aligned,
                          const unsigned* violated, int C, int R, float* weak, float* strong, void* stream) {
    if (n_pairs <= 0) return SGC_OK;
    SGC_LAUNCH(commonsense_flags_kernel, dim3((n_pairs * n_cand + 255) / 256), dim3(256), 0, (hipStream_t)stream, scat, ocat, cand_pred,
               n_pairs, n_cand, aligned, violated, C, R, weak, strong);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

int sgc_commonsense_filter(const long* scat, const long* pred, const long* ocat, float* conf, int n, const unsigned* aligned,
                           const unsigned* violated, int C, int R, void* stream) {
    if (n <= 0) return SGC_OK;
    SGC_LAUNCH(commonsense_filter_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, scat, pred, ocat, conf, n,
               aligned, violated, C, R);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

int sgc_overlap_filter(const int* bbox, const int* sub_idx, const int* obj_idx, unsigned char* out, int n_pairs, void* stream) {
    if (n_pairs <= 0) return SGC_OK;
    SGC_LAUNCH(overlap_filter_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, (hipStream_t)stream, bbox, sub_idx, obj_idx,
                       out, n_pairs);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

int sgc_topk_per_image(const float* conf, const int* seg_ptr, int n_img, int K, int* out_idx, int* out_count, void* stream) {
    if (K < 1 || K > 128) return SGC_ERR_ARG;
    if (n_img <= 0) return SGC_OK;
    SGC_LAUNCH(topk_kernel, dim3(n_img), dim3(256), 0, (hipStream_t)stream, conf, seg_ptr, K, out_idx, out_count);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

}  // extern "C"
