// Block-wide stable top-K selection, the one copy behind every per-image ranking: topk_kernel (csrc/kernels_eval.hip, 256
// threads, keys straight from the confidences) and scene_graph_topk_kernel (csrc/kernels_graph.hip, 1024 threads, keys cached in
// LDS).  Recall@K, the mined candidates, the predicted graphs and the RecallMeter counters all rest on the tie order fixed here.
#pragma once
#include "common.h"

__device__ __forceinline__ unsigned order_key(float f) {      // ascending uint order == ascending float order
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <int THREADS> struct TopkScratch {
    unsigned hist[256];
    unsigned prefix, mask;
    int remaining, cnt, base, wave_cnt[THREADS / 64];
    unsigned long long keys[128];                              // (~key << 32) | index, ascending = key descending, index ascending
};

// Every thread of a THREADS-wide workgroup calls this with the same n and k (0 <= k <= min(n, 128)); key_of(i) is the 32-bit key
// of element i < n and must give the same value every time it is asked.  Radix-select of the k-th largest key (4 x 8-bit LDS
// histograms), everything above it in any order plus the earliest ties by ordered compaction with wavefront ballots, bitonic sort
// of the <= 128 survivors: keys[0..k) end up as a stable descending argsort truncated to k, keys[k..128) as ~0.  Ends on a
// barrier, so the caller may read keys[] at once.
template <int THREADS, class KeyFn>
__device__ __forceinline__ void block_topk(TopkScratch<THREADS>& s, int n, int k, KeyFn key_of) {
    static_assert(THREADS >= 256 && THREADS % 64 == 0, "one thread per histogram bin, whole wavefronts");
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid < 128) s.keys[tid] = ~0ull;
    if (tid == 0) { s.prefix = 0; s.mask = 0; s.remaining = k; s.cnt = 0; }
    __syncthreads();
    if (k <= 0) return;
    for (int pass = 3; pass >= 0; --pass) {
        if (tid < 256) s.hist[tid] = 0;
        __syncthreads();
        const unsigned prefix = s.prefix, mask = s.mask;
        for (int i = tid; i < n; i += THREADS) {
            const unsigned key = key_of(i);
            if ((key & mask) == prefix) atomicAdd(&s.hist[(key >> (8 * pass)) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            int cum = 0, rem = s.remaining;
            for (int bk = 255; bk >= 0; --bk) {
                const int hv = (int)s.hist[bk];
                if (cum + hv >= rem) {
                    s.prefix = prefix | ((unsigned)bk << (8 * pass));
                    s.mask = mask | (0xffu << (8 * pass));
                    s.remaining = rem - cum;
                    break;
                }
                cum += hv;
            }
        }
        __syncthreads();
    }
    // thr is the k-th largest key: fewer than k keys lie above it, so the unordered positions stay inside keys[]
    const unsigned thr = s.prefix;
    for (int i = tid; i < n; i += THREADS) {
        const unsigned key = key_of(i);
        if (key > thr) {
            const int pos = atomicAdd(&s.cnt, 1);
            if (pos < 128) s.keys[pos] = ((unsigned long long)(~key) << 32) | (unsigned)i;
        }
    }
    __syncthreads();
    if (tid == 0) s.base = s.cnt;
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += THREADS) {
        if (s.base >= k) break;
        const int i = c0 + tid;
        const bool flag = i < n && key_of(i) == thr;
        const unsigned long long bal = __ballot(flag);
        const int within = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s.wave_cnt[wv] = __popcll(bal);
        __syncthreads();
        int off = s.base + within, total = 0;
        for (int w2 = 0; w2 < THREADS / 64; ++w2) {
            if (w2 < wv) off += s.wave_cnt[w2];
            total += s.wave_cnt[w2];
        }
        if (flag && off < k) s.keys[off] = ((unsigned long long)(~thr) << 32) | (unsigned)i;
        __syncthreads();
        if (tid == 0) s.base += total;
        __syncthreads();
    }
    // bitonic sort of 128 keys, ascending
    for (int size = 2; size <= 128; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            if (tid < 64) {
                const int lo = 2 * tid - (tid & (stride - 1));
                const int hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const unsigned long long a = s.keys[lo], bb = s.keys[hi];
                if ((a > bb) == up) { s.keys[lo] = bb; s.keys[hi] = a; }
            }
        }
    }
    __syncthreads();
}
