// What the exact neighbour searches share: the sorted set, its carve, the bound of a box and the lane of a walk (internal; the C ABI
// is include/ogs_knn.h).
//
// THE SORTED SET.  knn_sort_into_boxes (knn_neighbors.hip) is the front half of ogs_knn_neighbors and ogs_knn_dbscan, the whole of
// ogs_knn_index_build, and what groups the queries of ogs_knn_query and ogs_knn_radius_count:
//   bounding box -> 30-bit Morton keys -> four stable radix passes -> coordinates gathered into sorted order, NaN-padded to whole
//   BOXES of kKnnBox = 64 points, with the sorted ids and the axis-aligned bounds of every box.
//
// THE WALK.  One single-wave workgroup owns one RUN of kKnnBox consecutive sorted queries, one query per lane (KnnLane); the
// run is a box of its own set, so it has bounds.  Candidate boxes are tested 64 at a time, one per lane, by the lower bound of d2
// between the run's bounds and the candidate's (KnnLane::bound: the expression, and why it needs no margin), and a box is skipped only when that bound is STRICTLY above the
// walk's threshold.  A visited box is staged in LDS coordinate by coordinate and read with broadcast 16-byte reads, four points of
// one coordinate at a time; every lane tests its query against all 64 points with d2 = (dx*dx + dy*dy) + dz*dz (the files that
// hold a walk are compiled with -ffp-contract=off).  A padding lane or point has NaN coordinates and the id kNoId: its d2 is a
// NaN and compares false with everything.  Two kernels walk, each with a staging and a pair loop of its own:
//   knn_search_kernel (knn_search.hip)    the threshold is the largest K-th d2 of the wave's queries and falls; boxes are visited
//                                         outward from a start box
//   radius_walk_kernel (knn_radius.hip)   the threshold is fixed; boxes are visited in index order
#pragma once

#include "ogs_common.h"

#include <limits.h>

namespace ogs {

constexpr int kKnnBox = kWave;                          // points per box = queries per wave = candidates per staging round
constexpr int kKnnMaxK = 32;
constexpr int kBoundBlocks = 256;                       // workgroups (and partial records) of the bounding-box pass
constexpr int kNoId = INT_MAX;                          // id of an empty list slot and of a padding point: above every real id
static_assert(kBoundBlocks <= kBlock, "one thread folds one partial record");

constexpr int64_t knn_nbox(int64_t n) { return (n + kKnnBox - 1) / kKnnBox; }      // boxes of n points, runs of n queries
// a set the searches take: its padded rows and its box count fit an int
inline bool knn_size_ok(int64_t n) { return n >= 0 && n <= (int64_t)INT32_MAX - kKnnBox; }

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
    // the sorted set of n points; keyed: with first_key and frame (what a start box is found by)
    static KnnBoxes carve(Carver& c, int64_t n, bool keyed) {
        KnnBoxes b{};
        const size_t nbox = (size_t)knn_nbox(n), npad = nbox * kKnnBox;
        if (keyed) b.frame = c.take<float>(6);
        b.sx = c.take<float>(npad); b.sy = c.take<float>(npad); b.sz = c.take<float>(npad);
        b.sid = c.take<int32_t>(npad);
        b.box = c.take<float>(6 * nbox);
        if (keyed) b.first_key = c.take<uint32_t>(nbox);
        return b;
    }
};

// n in [1, INT32_MAX - kKnnBox]; pts [n, 3]; everything else as the structs say.  No read-back, nothing waits on another workgroup.
int knn_sort_into_boxes(int n, const float* pts, const KnnSortScratch& t, const KnnBoxes& out, hipStream_t s);

// The search (knn_search.hip): nruns runs of the sorted queries q against the nbox boxes of r, outward from box start[run]; K in
// [1, kKnnMaxK] rounds up to the next list size the search is compiled for.  One set against itself: q == r, start == nullptr
// (a run starts at itself), nruns == nbox.
int knn_launch_search(int nruns, int nbox, int K, int exclude_self, const KnnBoxes& q, const int32_t* start, const KnnBoxes& r,
                      int32_t* idx, float* d2, hipStream_t s);

// the persistent index of a point set (ogs_knn_index_build): what ogs_knn_query and ogs_knn_radius_count carve out of `index`
struct IndexLayout {
    KnnBoxes b;
    size_t bytes;
    static IndexLayout carve(void* p, int64_t n) {
        Carver c(p);
        IndexLayout t{};
        t.b = KnnBoxes::carve(c, n, true);
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

// tmp of a call that sorts one set and walks it: the sort's scratch and the set, unkeyed (ogs_knn_neighbors; with start, the queries
// of ogs_knn_query; without, those of ogs_knn_radius_count; ogs_knn_dbscan goes on carving from c)
struct SortedTmp {
    KnnSortScratch sort;
    KnnBoxes boxes;
    int32_t* start;                                     // [nbox] start box of every run; with_start only
    size_t bytes;
    static SortedTmp carve(Carver& c, int64_t n, bool with_start = false) {
        SortedTmp t{};
        t.sort = SortTmp::carve(c, n).sort;
        t.boxes = KnnBoxes::carve(c, n, false);
        if (with_start) t.start = c.take<int32_t>((size_t)knn_nbox(n));
        t.bytes = c.off;
        return t;
    }
};

// The front half of the two-set calls (knn_query.hip), after their own argument checks: tmp [tmp_bytes] is checked against
// SortedTmp of the m queries (the error names ogs_<name>_tmp_bytes), the index of n points is carved, read only from here on, and
// the queries are sorted into runs.
struct KnnTwoSets {
    KnnBoxes q, r;                                      // the queries in runs, the reference in boxes
    int32_t* start;                                     // [nruns], not filled; with_start only
    int nruns, nbox;
};
int knn_sort_queries(int64_t n, const void* index, int64_t m, const float* queries, void* tmp, size_t tmp_bytes, const char* name,
                     bool with_start, hipStream_t s, KnnTwoSets& out);

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

// One lane of a walk: its query and the bounds of its run.  Registers only.  (radius_walk_kernel keeps this set-up and the bound
// written out in its own text, for a measured reason it states; what it writes out must stay equal to these.)
struct KnnLane {
    float qx, qy, qz;                                   // NaN in a padding lane
    int qid;                                            // the query's row in the caller's order; kNoId in a padding lane
    bool valid;
    float qlo[3], qhi[3];                               // the run's bounds (wave-uniform)

    // lane `lane` of run `run` of the sorted set (qsx, qsy, qsz, qsid, qbox) of nruns runs
    __device__ __forceinline__ void load(int run, int nruns, int lane, const float* __restrict__ qsx, const float* __restrict__ qsy,
                                         const float* __restrict__ qsz, const int32_t* __restrict__ qsid,
                                         const float* __restrict__ qbox) {
        const size_t p = (size_t)run * kKnnBox + lane;
        qx = qsx[p]; qy = qsy[p]; qz = qsz[p];
        qid = qsid[p];
        valid = qid != kNoId;
#pragma unroll
        for (int a = 0; a < 3; ++a) { qlo[a] = qbox[(size_t)a * nruns + run]; qhi[a] = qbox[(size_t)(3 + a) * nruns + run]; }
    }

    // Lower bound of the computed fp32 d2 between any query of the run and any point of box c in [0, nbox) of
    // `box`: the d2 expression itself on the per-axis gaps g = max(lo_c - hi_q, lo_q - hi_c, 0).  It needs no safety margin.  For a
    // pair (q, p) of the two boxes and an axis where g > 0, say lo_c > hi_q: p >= lo_c and q <= hi_q, and the round-to-nearest
    // difference is monotone in either operand -- rounding maps a larger exact value to a larger or equal float, and is symmetric in
    // the sign -- so |q - p| as computed is >= lo_c - hi_q as computed, which is g; where g = 0 there is nothing to show.  All values are
    // then non-negative, where the rounded product and the rounded sum are monotone in both operands for the same reason, so each
    // term of (g0*g0 + g1*g1) + g2*g2 is <= the matching term of (dx*dx + dy*dy) + dz*dz, in the same order of operations -- which is
    // why the two must stay the same expression and uncontracted: an fma rounds once where the other side rounds twice.
    // fmaxf drops a NaN (a box of NaN points, inf - inf): that axis then contributes no gap and skips nothing; should a bound come
    // out a NaN all the same, every walk tests `!(lb > T)` and visits the box.
    __device__ __forceinline__ float bound(const float* __restrict__ box, int nbox, int c) const {
        float g[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float clo = box[(size_t)a * nbox + c], chi = box[(size_t)(3 + a) * nbox + c];
            g[a] = fmaxf(fmaxf(clo - qhi[a], qlo[a] - chi), 0.f);
        }
        return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    }
};

}  // namespace ogs
