// SGDET / SGCLS training targets: the ground-truth triples of a minibatch (pairs.sg_target_table's rows, sorted by image) assigned
// to the ordered pairs of the DETECTED objects' scene.  A row is a candidate of a pair under exactly the test that evaluation credits
// (reference evaluator.py:306-356 with predcls=False, as recall_accumulate_targets_kernel of csrc/kernels_metrics.hip restates it
// without the predicate): labels equal or equivalent (`equiv[target class][detection class]`), both rasterised-grid IoUs >= thr.  The
// pair's directed target (train_utils.py:169-187) is the predicate of its best candidate: the largest product of the two grid IoUs,
// compared in exact integer cell counts by 64-bit cross-multiplication (never two floats), the smallest row on a tie.  Everything is
// integer work on a few tens of rows per image: one thread per pair, plain loops.
#include "common.h"
#include "eval_geom.h"

struct AssignParams {
    const int* sub_idx; const int* obj_idx; const int* image; int P;          // [P] pair tables of the detected scene
    const int* pid; int pid_ld; const int* img_ptr;                          // [n_obj][pid_ld] pair of (subject, local object), [n_img+1]
    const long* cats; const float* boxes; int n_obj;                         // detections: classes, raw boxes [n_obj][4] (16-byte aligned)
    const int* t_ptr; int n_img;                                             // [n_img+1] rows of every image
    const long* t_rel; const long* t_scat; const long* t_ocat; const float* t_sbox; const float* t_obox; int n_t;
    const unsigned char* equiv; int n_equiv;
    int R, F; double iou_thresh;
    int* directed; int* raw; int* matched; int* target_hit;
};

// label_ok(t, c): the row is the target's class, the column the detection's (recall_accumulate_targets_kernel reads it so)
__device__ __forceinline__ bool label_ok(const AssignParams& p, long t, long c) {
    if (t == c) return true;
    return p.equiv && t >= 0 && t < p.n_equiv && c >= 0 && c < p.n_equiv && p.equiv[t * p.n_equiv + c];
}

// (intersection, union) of two rasterised rectangles in cells: the two integers box_iou_ok divides
__device__ __forceinline__ void inter_union(const GridBox a, const GridBox b, long& inter, long& uni) {
    inter = box_area(box_and(a, b));
    uni = box_area(a) + box_area(b) - inter;
}

__global__ __launch_bounds__(256) void assign_pair_targets_kernel(const AssignParams p) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= p.P) return;
    int best = -1, best_rel = -1;
    long best_num = 0, best_den = 0;                                         // q(best) = best_num / best_den
    const int img = p.image[row], s = p.sub_idx[row], o = p.obj_idx[row];
    if (p.n_t > 0 && img >= 0 && img < p.n_img && s >= 0 && s < p.n_obj && o >= 0 && o < p.n_obj) {
        const long sc = p.cats[s], oc = p.cats[o];
        const GridBox sb = load_box(p.boxes, s, p.F), ob = load_box(p.boxes, o, p.F);
        const int t0 = max(p.t_ptr[img], 0), t1 = min(p.t_ptr[img + 1], p.n_t);
        for (int t = t0; t < t1; ++t) {
            const long rel = p.t_rel[t];
            if (rel < 0 || rel >= p.R || !label_ok(p, p.t_scat[t], sc) || !label_ok(p, p.t_ocat[t], oc)) continue;
            const GridBox tsb = load_box(p.t_sbox + 4L * t, p.F), tob = load_box(p.t_obox + 4L * t, p.F);
            if (!box_iou_ok(sb, tsb, p.iou_thresh) || !box_iou_ok(ob, tob, p.iou_thresh)) continue;
            p.target_hit[t] = 1;                                             // idempotent: every writer stores the same value
            long is, us, io, uo;
            inter_union(sb, tsb, is, us);
            inter_union(ob, tob, io, uo);
            const long num = is * io, den = us * uo;                         // <= F^4 = 2^28 each for F <= 128: the cross products fit 64 bits
            if (best < 0 || num * best_den > best_num * den) {               // strictly better only: the smallest row wins a tie
                best = t; best_rel = (int)rel; best_num = num; best_den = den;
            }
        }
    }
    p.matched[row] = best;
    p.directed[row] = best_rel;
}

// raw[p] = directed[p] if the pair is connected, else the directed target of the reversed pair (pid[object][local subject]): what
// sgc_scene_tables' `raw` is in PredCLS, the stored predicate of the unordered pair.
__global__ __launch_bounds__(256) void assign_raw_targets_kernel(const AssignParams p) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= p.P) return;
    int r = p.directed[row];
    if (r < 0) {
        const int img = p.image[row], s = p.sub_idx[row], o = p.obj_idx[row];
        if (img >= 0 && img < p.n_img && s >= 0 && s < p.n_obj && o >= 0 && o < p.n_obj) {
            const int local = s - p.img_ptr[img];
            if (local >= 0 && local < p.pid_ld) {
                const int rev = p.pid[(long)o * p.pid_ld + local];
                if (rev >= 0 && rev < p.P) r = p.directed[rev];
            }
        }
    }
    p.raw[row] = r;
}

extern "C" {

int sgc_assign_pair_targets(const int* sub_idx, const int* obj_idx, const int* image, int n_pairs, const int* pid, int pid_ld,
                            const int* img_ptr, const long* cats, const float* boxes, int n_obj, const int* t_ptr, int n_img,
                            const long* t_rel, const long* t_scat, const long* t_ocat, const float* t_sbox, const float* t_obox,
                            int n_targets, const unsigned char* equiv, int n_equiv, int R, int feature_size, double iou_thresh,
                            int* directed, int* raw, int* matched, int* target_hit, void* stream) {
    if (n_pairs < 0 || n_targets < 0 || n_img < 0 || n_obj < 0 || pid_ld < 0 || R < 1 || feature_size < 1 || feature_size > 128 ||
        !(iou_thresh >= 0.0) || (equiv && n_equiv < 1))
        return SGC_ERR_ARG;
    if (n_targets > 0) {
        if (!t_ptr || !t_rel || !t_scat || !t_ocat || !t_sbox || !t_obox || !target_hit || n_img < 1) return SGC_ERR_ARG;
        if (hipMemsetAsync(target_hit, 0, sizeof(int) * (size_t)n_targets, (hipStream_t)stream) != hipSuccess) return SGC_ERR_LAUNCH;
    }
    if (n_pairs == 0) return SGC_OK;
    if (!sub_idx || !obj_idx || !image || !pid || !img_ptr || !cats || !boxes || !directed || !raw || !matched || n_img < 1 ||
        n_obj < 1 || pid_ld < 1)
        return SGC_ERR_ARG;
    const AssignParams p{sub_idx, obj_idx, image, n_pairs, pid, pid_ld, img_ptr, cats, boxes, n_obj, t_ptr, n_img, t_rel, t_scat, t_ocat,
                         t_sbox, t_obox, n_targets, equiv, equiv ? n_equiv : 0, R, feature_size, iou_thresh, directed, raw, matched,
                         target_hit};
    const dim3 grid((unsigned)((n_pairs + 255) / 256));
    SGC_LAUNCH(assign_pair_targets_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    SGC_CHECK_LAUNCH();
    SGC_LAUNCH(assign_raw_targets_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);      // same stream: every directed is written
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

}  // extern "C"
