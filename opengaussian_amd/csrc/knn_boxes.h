// What the exact neighbour searches share: the sorted-box front half and the search kernel (internal; the C ABI is
// include/ogs_knn.h).
//
// knn_sort_into_boxes (knn_neighbors.hip) is the front half of ogs_knn_neighbors, the whole of ogs_knn_index_build, and what groups
// the queries of ogs_knn_query:
//   bounding box -> 30-bit Morton keys -> four stable radix passes -> coordinates gathered into sorted order, NaN-padded to whole
//   boxes of kKnnBox points, with the sorted ids and the axis-aligned bounds of every box.
// knn_search_kernel is the search both run: a wave of 64 queries, one per lane, against boxes visited outward from a start box.
#pragma once

#include "ogs_common.h"

#include <limits.h>

namespace ogs {

constexpr int kKnnBox = kWave;                          // points per box = queries per wave = candidates per staging round
constexpr int kKnnMaxK = 32;
constexpr int kBoundBlocks = 256;                       // workgroups (and partial records) of the bounding-box pass
constexpr int kNoId = INT_MAX;                          // id of an empty list slot and of a padding point: above every real id
static_assert(kBoundBlocks <= kBlock, "one thread folds one partial record");

struct KnnSortScratch {                                 // only needed while knn_sort_into_boxes runs
    float* partial;                                     // [kBoundBlocks][6] min xyz, max xyz
    uint32_t* keys[2];                                  // [n] Morton keys, ping-pong; keys[0] holds the sorted keys at the end
    uint32_t* vals[2];                                  // [n] point ids, ping-pong; vals[0] holds the sorted order at the end
    void* sort_tmp;                                     // sort_tmp_bytes(n)
};

struct KnnBoxes {                                       // what a search reads of a point set
    float *sx, *sy, *sz;                                // [nbox * kKnnBox] sorted coordinates, NaN past n
    int32_t* sid;                                       // [nbox * kKnnBox] sorted ids (clamped to [0, n)), kNoId past n
    float* box;                                         // [6][nbox] min xyz, max xyz of every box
    uint32_t* first_key;                                // [nbox] Morton key of every box's first point; may be nullptr
    float* frame;                                       // [6] min xyz, max xyz of the set: the frame of its keys; may be nullptr
};

// n in [1, INT32_MAX - kKnnBox]; pts [n, 3]; everything else as the structs say.  No read-back, nothing waits on another workgroup.
int knn_sort_into_boxes(int n, const float* pts, const KnnSortScratch& t, const KnnBoxes& out, hipStream_t s);

// the persistent index of a point set (ogs_knn_index_build): what ogs_knn_query and ogs_knn_radius_count carve out of `index`
struct IndexLayout {
    KnnBoxes b;
    size_t bytes;
    static IndexLayout carve(void* p, int64_t n) {
        Carver c(p);
        IndexLayout t{};
        const size_t nbox = (size_t)((n + kKnnBox - 1) / kKnnBox), npad = nbox * kKnnBox;
        t.b.frame = c.take<float>(6);
        t.b.sx = c.take<float>(npad); t.b.sy = c.take<float>(npad); t.b.sz = c.take<float>(npad);
        t.b.sid = c.take<int32_t>(npad);
        t.b.box = c.take<float>(6 * nbox);
        t.b.first_key = c.take<uint32_t>(nbox);
        t.bytes = c.off;
        return t;
    }
};

// the scratch of one knn_sort_into_boxes call over n points
struct SortTmp {
    KnnSortScratch sort;
    size_t bytes;
    static SortTmp carve(Carver& c, int64_t n) {
        SortTmp t{};
        t.sort.partial = c.take<float>((size_t)kBoundBlocks * 6);
        for (int i = 0; i < 2; ++i) { t.sort.keys[i] = c.take<uint32_t>((size_t)n); t.sort.vals[i] = c.take<uint32_t>((size_t)n); }
        t.sort.sort_tmp = c.take<char>(sort_tmp_bytes(n));
        t.bytes = c.off;
        return t;
    }
};

__device__ __forceinline__ float wave_min_f(float v) {
    for (int m = kWave / 2; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, kWave));
    return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
    for (int m = kWave / 2; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, kWave));
    return v;
}

__device__ __forceinline__ uint32_t spread10(uint32_t v) {       // abcdefghij -> a00b00c00...j
    v &= 1023u;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// cell of a coordinate: always in [0, 1023] -- a NaN or an infinity anywhere in the chain ends as 0 or 1023
__device__ __forceinline__ uint32_t knn_cell(float v, float lo, float scale) {
    const float t = (v - lo) * scale;
    return (uint32_t)(int)fminf(fmaxf(t, 0.f), 1023.f);            // fmaxf(NaN, 0) = 0
}

// 30-bit Morton key of p in the frame [lo, hi]: 10 bits per axis, a point outside the frame lands in a boundary cell
__device__ __forceinline__ uint32_t knn_morton(const float (&p)[3], const float (&lo)[3], const float (&hi)[3]) {
    uint32_t key = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float ext = hi[a] - lo[a];
        const float scale = ext > 0.f && ext < INFINITY ? 1024.f / ext : 0.f;      // a zero extent: every point in cell 0
        key |= spread10(knn_cell(p[a], lo[a], scale)) << a;
    }
    return key;
}

// (d, j) before (bd, bi) in the order (d2, id)
__device__ __forceinline__ bool knn_before(float d, int j, float bd, int bi) {
    return d < bd || (d == bd && j < bi);
}

// offset o of the outward walk: 0, +1, -1, +2, -2, ...
__device__ __forceinline__ int knn_delta(int o) { return (o & 1) ? (o + 1) >> 1 : -(o >> 1); }

#ifndef OGS_KNN_BOXES_NO_SEARCH     // knn_radius.hip walks the boxes with a kernel of its own and wants no copy of this one
namespace {        // internal linkage: every file that includes this builds and registers its own copy of the kernel (no -fgpu-rdc)

// The search: one single-wave workgroup per RUN of kKnnBox queries (gridDim.x runs), one query per lane.  The queries are the
// sorted set (qsx, qsy, qsz, qsid, qbox) -- NaN coordinates and qsid = kNoId in a padding lane, where nothing is ever inserted --
// and the candidates the sorted set (sx, sy, sz, sid, box) of nbox boxes; ogs_knn_neighbors passes the same set twice.  The
// candidate boxes are visited outward in sorted order from a start box: start[run] (clamped to [0, nbox)), or, with
// start == nullptr, box `run` itself (one set: the run IS that box).  64 candidates at a time, one per lane, are tested against
// the run's bounds, and a box is skipped when its lower bound is STRICTLY above the largest K-th d2 of the wave's queries (an
// equal distance with a smaller id still displaces).  The lower bound is the d2 expression itself on the per-axis gaps
// max(lo_c - hi_q, lo_q - hi_c, 0): round-to-nearest subtraction, product and sum are monotone, so the bound is <= the computed
// fp32 d2 of every pair of the two boxes and needs no safety margin -- wherever the walk starts: it reaches every box, and the
// start only decides how fast the threshold falls.  A visited box is staged in LDS coordinate by coordinate and read with
// broadcast 16-byte reads, four points of one coordinate at a time.  With exclude_self a candidate whose id is the query's own
// is left out.  Row qsid of idx_out / d2_out [*, K] takes the first K pairs of the lane's list; an empty slot is (-1, +inf).
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
    const size_t p = (size_t)run * kKnnBox + lane;
    const float qx = qsx[p], qy = qsy[p], qz = qsz[p];
    const int qid = qsid[p];
    const bool valid = qid != kNoId;
    const int self = exclude_self ? qid : -1;
    float qlo[3], qhi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { qlo[a] = qbox[(size_t)a * nruns + run]; qhi[a] = qbox[(size_t)(3 + a) * nruns + run]; }

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
        float lb = 0.f;
        if (inside) {
            float g[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float clo = box[(size_t)a * nbox + c], chi = box[(size_t)(3 + a) * nbox + c];
                g[a] = fmaxf(fmaxf(clo - qhi[a], qlo[a] - chi), 0.f);
            }
            lb = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
        }
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
                    const float dx = qx - xs[u], dy = qy - ys[u], dz = qz - zs[u];
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
            T = wave_max_f(valid ? kth : -INFINITY);
        }
    }
    if (!valid) return;
    const size_t o = (size_t)qid * (size_t)K;                      // qid in [0, rows of the query set): clamped by the gather
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

// nruns runs of the sorted queries q against the nbox boxes of r; K in [1, kKnnMaxK] rounds up to the next list size the search
// is compiled for.  One set against itself: q == r, start == nullptr, nruns == nbox.
int knn_launch_search(int nruns, int nbox, int K, int exclude_self, const KnnBoxes& q, const int32_t* start, const KnnBoxes& r,
                      int32_t* idx, float* d2, hipStream_t s) {
    if (K <= 4) return knn_launch_search_lists<4>(nruns, nbox, K, exclude_self, q, start, r, idx, d2, s);
    if (K <= 8) return knn_launch_search_lists<8>(nruns, nbox, K, exclude_self, q, start, r, idx, d2, s);
    if (K <= 16) return knn_launch_search_lists<16>(nruns, nbox, K, exclude_self, q, start, r, idx, d2, s);
    return knn_launch_search_lists<32>(nruns, nbox, K, exclude_self, q, start, r, idx, d2, s);
}

}  // namespace
#endif

}  // namespace ogs
