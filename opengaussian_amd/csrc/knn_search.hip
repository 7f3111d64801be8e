// The K-nearest search over sorted boxes: the one kernel behind ogs_knn_neighbors and ogs_knn_query (declared in knn_boxes.h, which
// describes the walk it shares with knn_radius.hip).
//
// A lane keeps its K best (d2, id) pairs in registers as a sorted list (templated on 4 / 8 / 16 / 32; a requested K rounds up and
// the first K pairs are stored).  The threshold of the walk is T, the largest K-th d2 of the wave's queries: a box is skipped when
// its lower bound is STRICTLY above T (an equal distance with a smaller id still displaces), and T only falls.  So the boxes are
// visited OUTWARD in sorted order from a start box, nearest first in Morton order, to bring T down early -- and wherever the walk
// starts it reaches every box: the start only decides how fast the threshold falls, never the result.  The order (d2, id) is
// total, so the lists are unique and do not depend on the order of the visits.  A cloud that cannot be pruned (all points
// coincident: every bound and every K-th value is 0) visits every box: one brute pass over all pairs, still correct.
//
// This file is compiled with -ffp-contract=off: d2 = (dx*dx + dy*dy) + dz*dz, exactly so, and a lower bound that is monotone.
#include "knn_boxes.h"

namespace ogs {
namespace {

// offset o of the outward walk: 0, +1, -1, +2, -2, ...
__device__ __forceinline__ int knn_delta(int o) { return (o & 1) ? (o + 1) >> 1 : -(o >> 1); }

// One single-wave workgroup per RUN of kKnnBox queries (gridDim.x runs), one query per lane.  The queries are the sorted set
// (qsx, qsy, qsz, qsid, qbox) -- nothing is ever inserted in a padding lane -- and the candidates the sorted set (sx, sy, sz,
// sid, box) of nbox boxes; ogs_knn_neighbors passes the same set twice.  The start box is start[run] (clamped to [0, nbox)), or,
// with start == nullptr, box `run` itself (one set: the run IS that box).  With exclude_self a candidate whose id is the query's
// own is left out.  Row qsid of idx_out / d2_out [*, K] takes the first K pairs of the lane's list; an empty slot is (-1, +inf).
template <int KT>
__global__ __launch_bounds__(kKnnBox) void knn_search_kernel(int nbox, int K, int exclude_self, const float* __restrict__ qsx,
                                                             const float* __restrict__ qsy, const float* __restrict__ qsz,
                                                             const int32_t* __restrict__ qsid, const float* __restrict__ qbox,
                                                             const int32_t* __restrict__ start, const float* __restrict__ sx,
                                                             const float* __restrict__ sy, const float* __restrict__ sz,
                                                             const int32_t* __restrict__ sid, const float* __restrict__ box,
                                                             int32_t* __restrict__ idx_out, float* __restrict__ d2_out) {
    __shared__ __attribute__((aligned(16))) float cx[kKnnBox], cy[kKnnBox], cz[kKnnBox];
    __shared__ __attribute__((aligned(16))) int cid[kKnnBox];
    const int lane = threadIdx.x, run = blockIdx.x, nruns = gridDim.x;
    const int b = start ? min(max(start[run], 0), nbox - 1) : run;
    KnnLane q;
    q.load(run, nruns, lane, qsx, qsy, qsz, qsid, qbox);
    const int self = exclude_self ? q.qid : -1;

    float bd[KT];
    int bi[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) { bd[k] = INFINITY; bi[k] = kNoId; }

    float T = INFINITY;                                            // largest K-th d2 among the wave's queries
    const int reach = max(b, nbox - 1 - b);                        // |delta| of the farthest box
    for (int o0 = 0; o0 <= 2 * reach; o0 += kKnnBox) {
        // ---- 64 candidate boxes, one per lane: the lower bound of d2 between the two boxes --------------------------------
        const int c = b + knn_delta(o0 + lane);
        const bool inside = c >= 0 && c < nbox;
        const float lb = inside ? q.bound(box, nbox, c) : 0.f;
        unsigned long long todo = __ballot(inside && !(lb > T));    // (a NaN bound is visited)
        while (todo) {
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1;
            const float lbl = __shfl(lb, l, kWave);
            if (lbl > T) continue;                                 // T has fallen since the ballot (wave-uniform)
            const int cb = b + knn_delta(o0 + l);                  // in [0, nbox): lane l was `inside`
            // ---- stage the box, then every query against its 64 points -----------------------------------------------------
            const size_t cp = (size_t)cb * kKnnBox + lane;
            const float lx = sx[cp], ly = sy[cp], lz = sz[cp];
            const int lid = sid[cp];
            __syncthreads();                                       // the previous box has been consumed
            cx[lane] = lx; cy[lane] = ly; cz[lane] = lz; cid[lane] = lid;
            __syncthreads();
#pragma unroll 2
            for (int v = 0; v < kKnnBox; v += 4) {
                const float4 x4 = *reinterpret_cast<const float4*>(cx + v);
                const float4 y4 = *reinterpret_cast<const float4*>(cy + v);
                const float4 z4 = *reinterpret_cast<const float4*>(cz + v);
                const int4 i4 = *reinterpret_cast<const int4*>(cid + v);
                const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, ys[4] = {y4.x, y4.y, y4.z, y4.w}, zs[4] = {z4.x, z4.y, z4.z, z4.w};
                const int js[4] = {i4.x, i4.y, i4.z, i4.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float dx = q.qx - xs[u], dy = q.qy - ys[u], dz = q.qz - zs[u];
                    const float d = (dx * dx + dy * dy) + dz * dz;  // NaN for a padding point: before nothing
                    const int j = js[u];
                    if (knn_before(d, j, bd[KT - 1], bi[KT - 1]) && j != self) {
                        // slot k takes the candidate where it goes before slot k but not before slot k - 1, and the old
                        // slot k - 1 where it goes before both; static indices only
#pragma unroll
                        for (int k = KT - 1; k >= 1; --k) {
                            const bool here = knn_before(d, j, bd[k], bi[k]), above = knn_before(d, j, bd[k - 1], bi[k - 1]);
                            bd[k] = here ? (above ? bd[k - 1] : d) : bd[k];
                            bi[k] = here ? (above ? bi[k - 1] : j) : bi[k];
                        }
                        if (knn_before(d, j, bd[0], bi[0])) { bd[0] = d; bi[0] = j; }
                    }
                }
            }
            float kth = bd[KT - 1];
#pragma unroll
            for (int k = 0; k < KT - 1; ++k) kth = k == K - 1 ? bd[k] : kth;
            T = wave_max_f(q.valid ? kth : -INFINITY);
        }
    }
    if (!q.valid) return;
    const size_t o = (size_t)q.qid * (size_t)K;                    // qid in [0, rows of the query set): clamped by the gather
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        if (k < K) {
            const bool filled = bi[k] != kNoId;
            idx_out[o + k] = filled ? bi[k] : -1;
            d2_out[o + k] = filled ? bd[k] : INFINITY;
        }
    }
}

template <int KT>
int knn_launch_search_lists(int nruns, int nbox, int K, int exclude_self, const KnnBoxes& q, const int32_t* start,
                            const KnnBoxes& r, int32_t* idx, float* d2, hipStream_t s) {
    OGS_LAUNCH(knn_search_kernel<KT>, dim3((unsigned)nruns), dim3(kKnnBox), 0, s, nbox, K, exclude_self, q.sx, q.sy, q.sz, q.sid,
               q.box, start, r.sx, r.sy, r.sz, r.sid, r.box, idx, d2);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

}  // namespace

int knn_launch_search(int nruns, int nbox, int K, int exclude_self, const KnnBoxes& q, const int32_t* start, const KnnBoxes& r,
                      int32_t* idx, float* d2, hipStream_t s) {
    if (K <= 4) return knn_launch_search_lists<4>(nruns, nbox, K, exclude_self, q, start, r, idx, d2, s);
    if (K <= 8) return knn_launch_search_lists<8>(nruns, nbox, K, exclude_self, q, start, r, idx, d2, s);
    if (K <= 16) return knn_launch_search_lists<16>(nruns, nbox, K, exclude_self, q, start, r, idx, d2, s);
    return knn_launch_search_lists<32>(nruns, nbox, K, exclude_self, q, start, r, idx, d2, s);
}

}  // namespace ogs
