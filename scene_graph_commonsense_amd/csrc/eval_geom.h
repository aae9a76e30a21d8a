// Shared device pieces of the evaluation kernels (csrc/kernels_eval.hip, kernels_graph.hip, kernels_metrics.hip): the triplet-set
// lookup, the rasterised-box geometry of the grid IoU, and the first-matching-rank scan of one wavefront.
#pragma once
#include "common.h"

// A set of (subject class s, predicate r, object class o) triplets is a bitmap of C*R*C bits in 32-bit words: triplet (s, r, o)
// is bit (s*R + r)*C + o, bit b of the set is bit (b & 31) of word b >> 5.  commonsense.TripletBitmaps._pack writes this layout.
// A label outside [0, C) or [0, R) is in no set.
// triplet_bits looks one triplet up in two sets of one shape under one range check (bit 0 of the result: in `a`, bit 1: in `b`);
// the sites that read the aligned and the violated set use it, because two calls of triplet_bit compile to two range checks and
// two index products (12 VGPRs against 9 in commonsense_flags_kernel).
__device__ __forceinline__ unsigned triplet_bits(const unsigned* a, const unsigned* b, long s, long r, long o, int C, int R) {
    if (s < 0 || s >= C || o < 0 || o >= C || r < 0 || r >= R) return 0u;
    const long bit = (s * R + r) * C + o, w = bit >> 5;
    return ((a[w] >> (bit & 31)) & 1u) | (((b[w] >> (bit & 31)) & 1u) << 1);
}
__device__ __forceinline__ bool triplet_bit(const unsigned* map, long s, long r, long o, int C, int R) {
    return triplet_bits(map, map, s, r, o, C, R) & 1u;
}

struct GridBox { int x0, x1, y0, y1; };                                // half-open, after int() truncation and slice clipping

__device__ __forceinline__ int slice_clip(float v, int F) {           // mask[int(a):int(b)] on an axis of length F: int(v), then Python slice clipping
    const int i = (int)v;
    return i < 0 ? max(i + F, 0) : min(i, F);
}
__device__ __forceinline__ GridBox load_box(const float* __restrict__ boxes, int o, int F) {      // row o of a 16-byte aligned [n][4] f32 table: one 16-byte load
    const f32x4 b = *reinterpret_cast<const f32x4*>(boxes + 4L * o);
    return GridBox{slice_clip(b[0], F), slice_clip(b[1], F), slice_clip(b[2], F), slice_clip(b[3], F)};
}
__device__ __forceinline__ GridBox load_box(const float* __restrict__ row, int F) {               // one row (x0,x1,y0,y1) of any alignment: four loads
    return GridBox{slice_clip(row[0], F), slice_clip(row[1], F), slice_clip(row[2], F), slice_clip(row[3], F)};
}
// An empty box (x1 <= x0 or y1 <= y0) stays empty under box_and, so its area is 0 without a special case.
__device__ __forceinline__ GridBox box_and(const GridBox a, const GridBox b) {
    return GridBox{max(a.x0, b.x0), min(a.x1, b.x1), max(a.y0, b.y0), min(a.y1, b.y1)};
}
__device__ __forceinline__ int box_area(const GridBox a) { return max(a.x1 - a.x0, 0) * max(a.y1 - a.y0, 0); }

// IoU of two rasterised rectangles >= thr; union == 0 -> IoU 0 (evaluator.py:84-94).  "Either area is 0, so the intersection is
// 0" (evaluator.grid_iou_matrix spells it out) needs no branch here: box_and of an empty rectangle is empty.
__device__ __forceinline__ bool box_iou_ok(const GridBox a, const GridBox b, double thr) {
    const int aa = box_area(a), ab = box_area(b), inter = box_area(box_and(a, b));
    const int uni = aa + ab - inter;
    const double iou = uni > 0 ? (double)inter / (double)uni : 0.0;
    return iou >= thr;
}
// |X & (ts | to)| for a rectangle X: inclusion-exclusion over rectangles, whose intersections are rectangles again
__device__ __forceinline__ int area_in_pair(const GridBox x, const GridBox ts, const GridBox to) {
    const GridBox xs = box_and(x, ts);
    return box_area(xs) + box_area(box_and(x, to)) - box_area(box_and(xs, to));
}
// IoU of the masks (subject | object) of a prediction and of a target >= thr (evaluator.py:97-115), in exact cell counts on a grid
// of any size: |P & T| = |S & T| + |O & T| - |S & O & T| with every term a sum of rectangle areas.  union == 0 -> IoU 0.
__device__ __forceinline__ bool union_iou_ok(const GridBox s, const GridBox o, const GridBox ts, const GridBox to, double thr) {
    const GridBox so = box_and(s, o);
    const int inter = area_in_pair(s, ts, to) + area_in_pair(o, ts, to) - area_in_pair(so, ts, to);
    const int ap = box_area(s) + box_area(o) - box_area(so);
    const int at = box_area(ts) + box_area(to) - box_area(box_and(ts, to));
    const int uni = ap + at - inter;
    const double iou = uni > 0 ? (double)inter / (double)uni : 0.0;
    return iou >= thr;
}

// The lowest rank j < cnt with ok(j), or `none`.  A whole wavefront calls this with the same cnt: lane l tests ranks l, l + 64,
// ...; a ballot gives the first match of each trip, and the first trip with a match ends the scan.
template <class OkFn> __device__ __forceinline__ int first_match_rank(int cnt, int none, OkFn ok) {
    const int lane = threadIdx.x & 63;
    for (int j0 = 0; j0 < cnt; j0 += 64) {
        const int j = j0 + lane;
        const unsigned long long m = __ballot(j < cnt && ok(j));
        if (m) return j0 + __ffsll((long long)m) - 1;
    }
    return none;
}
