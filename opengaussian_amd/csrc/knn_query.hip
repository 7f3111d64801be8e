// Exact K nearest neighbours BETWEEN TWO point sets: a persistent index of the reference set, queried many times
// (include/ogs_knn.h: ogs_knn_index_build, ogs_knn_query).
//
// ogs_knn_index_build is the front half of ogs_knn_neighbors (knn_sort_into_boxes, knn_boxes.h) run on the reference set and kept:
// the sorted coordinates in boxes of kKnnBox = 64 points, the sorted ids, the bounds of every box, the Morton key of every box's
// first point and the bounding box that made the keys (the reference's FRAME).  A copy: `points` is not read again.
//
// ogs_knn_query:
//   1. GROUPING.  The same front half on the queries, keyed in the queries' OWN bounding box: runs of 64 consecutive sorted
//      queries are spatially coherent wherever the queries lie -- keyed in the reference's frame, every query outside it would
//      collapse into a boundary cell and a run would span the whole outside.
//   2. START BOX.  Per run, its median query (the middle of the run in sorted order) is keyed in the REFERENCE's frame (clamped
//      to its boundary cells when outside) and located among the per-box first keys by bisection: the last box whose first key
//      is not above it, clamped to [0, nbox).  One thread per run, at most 32 steps.  (The centre of the run's bounds was the
//      first choice and measured slower: a run that straddles a jump of the Morton curve has its centre far from both halves.)
//   3. SEARCH.  knn_search_kernel (knn_boxes.h), the kernel of ogs_knn_neighbors: one wave owns one run, one query per lane,
//      K-best lists in registers, reference boxes visited outward from the start box, 64 lower bounds per round between the
//      run's bounds and the candidate box's bounds.  The walk reaches every box and skips one only when its bound is strictly above the largest
//      K-th d2 of the wave, so the result does not depend on the start box; the start only decides how fast that threshold falls.
//
// No read-back, no float atomics, nothing waits on another workgroup.
// This file is compiled with -ffp-contract=off: d2 = (dx*dx + dy*dy) + dz*dz, exactly so, and a lower bound that is monotone.
#include "knn_boxes.h"
#include "../../include/ogs_knn.h"

namespace ogs {
namespace {

struct QueryTmp {
    KnnSortScratch sort;
    KnnBoxes runs;                                      // the queries in runs of kKnnBox; no first_key, no frame
    int32_t* start;                                     // [nruns] start box of every run
    size_t bytes;
    static QueryTmp carve(void* p, int64_t m) {
        Carver c(p);
        QueryTmp t{};
        const size_t nruns = (size_t)((m + kKnnBox - 1) / kKnnBox), npad = nruns * kKnnBox;
        t.sort = SortTmp::carve(c, m).sort;
        t.runs.sx = c.take<float>(npad); t.runs.sy = c.take<float>(npad); t.runs.sz = c.take<float>(npad);
        t.runs.sid = c.take<int32_t>(npad);
        t.runs.box = c.take<float>(6 * nruns);
        t.start = c.take<int32_t>(nruns);
        t.bytes = c.off;
        return t;
    }
};

__global__ __launch_bounds__(kBlock) void knn_start_kernel(int m, int nruns, int nbox, const float* __restrict__ qsx,
                                                           const float* __restrict__ qsy, const float* __restrict__ qsz,
                                                           const float* __restrict__ frame,
                                                           const uint32_t* __restrict__ first_key, int32_t* __restrict__ start) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= nruns) return;
    const size_t mid_q = (size_t)r * kKnnBox + (min(kKnnBox, m - r * kKnnBox) - 1) / 2;      // the run's median query: never padding
    const float p[3] = {qsx[mid_q], qsy[mid_q], qsz[mid_q]};
    float lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = frame[a]; hi[a] = frame[3 + a]; }
    const uint32_t key = knn_morton(p, lo, hi);
    int below = 0, end = nbox;                                     // boxes [0, below) have a first key <= key, [end, nbox) above
    for (int step = 0; step < 32 && below < end; ++step) {
        const int mid = below + ((end - below) >> 1);              // in [below, end): inside [0, nbox)
        if (first_key[mid] <= key) below = mid + 1; else end = mid;
    }
    start[r] = min(max(below - 1, 0), nbox - 1);
}

__global__ __launch_bounds__(kBlock) void knn_empty_lists_kernel(int64_t total, int32_t* __restrict__ idx, float* __restrict__ d2) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total) return;
    idx[e] = -1;
    d2[e] = INFINITY;
}

bool size_ok(int64_t n) { return n >= 0 && n <= (int64_t)INT32_MAX - kKnnBox; }

}  // namespace
}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_knn_index_bytes(int64_t n) {
    if (n <= 0 || !size_ok(n)) return 0;
    return IndexLayout::carve(nullptr, n).bytes;
}

size_t ogs_knn_index_build_tmp_bytes(int64_t n) {
    if (n <= 0 || !size_ok(n)) return 0;
    Carver c(nullptr);
    return SortTmp::carve(c, n).bytes;
}

int ogs_knn_index_build(int64_t n, const float* points, void* index, size_t index_bytes, void* tmp, size_t tmp_bytes,
                        void* stream_) {
    if (!size_ok(n)) {
        set_error("knn_index_build: bad size (n=%lld; 0 <= n <= INT32_MAX - %d)", (long long)n, kKnnBox);
        return OGS_ERR_INVALID_ARG;
    }
    if (n == 0) return OGS_OK;
    if (!points || !index || !tmp) { set_error("knn_index_build: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    const IndexLayout ix = IndexLayout::carve(index, n);
    if (index_bytes < ix.bytes) {
        set_error("knn_index_build: index has %zu bytes, %zu needed (ogs_knn_index_bytes)", index_bytes, ix.bytes);
        return OGS_ERR_INVALID_ARG;
    }
    Carver c(tmp);
    const SortTmp t = SortTmp::carve(c, n);
    if (tmp_bytes < t.bytes) {
        set_error("knn_index_build: tmp has %zu bytes, %zu needed (ogs_knn_index_build_tmp_bytes)", tmp_bytes, t.bytes);
        return OGS_ERR_INVALID_ARG;
    }
    return knn_sort_into_boxes((int)n, points, t.sort, ix.b, static_cast<hipStream_t>(stream_));
}

size_t ogs_knn_query_tmp_bytes(int64_t n, int64_t m) {
    if (n <= 0 || m <= 0 || !size_ok(n) || !size_ok(m)) return 0;
    return QueryTmp::carve(nullptr, m).bytes;
}

int ogs_knn_query(int64_t n, const void* index, int64_t m, const float* queries, int32_t K, int32_t* idx, float* d2, void* tmp,
                  size_t tmp_bytes, void* stream_) {
    if (!size_ok(n) || !size_ok(m) || K < 1 || K > kKnnMaxK || m * (int64_t)K >= ((int64_t)1 << 31)) {
        set_error("knn_query: bad sizes (n=%lld m=%lld K=%d; 1 <= K <= %d, m * K < 2^31)", (long long)n, (long long)m, K, kKnnMaxK);
        return OGS_ERR_INVALID_ARG;
    }
    if (m == 0) return OGS_OK;
    if (!idx || !d2) { set_error("knn_query: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (n == 0) {                                                  // no candidate: every list is empty
        const int64_t total = m * K;
        OGS_LAUNCH(knn_empty_lists_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, total, idx, d2);
        OGS_LAUNCH_CHECK(0, s);
        return OGS_OK;
    }
    if (!index || !queries || !tmp) { set_error("knn_query: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    const QueryTmp q = QueryTmp::carve(tmp, m);
    if (tmp_bytes < q.bytes) {
        set_error("knn_query: tmp has %zu bytes, %zu needed (ogs_knn_query_tmp_bytes)", tmp_bytes, q.bytes);
        return OGS_ERR_INVALID_ARG;
    }
    const KnnBoxes r = IndexLayout::carve(const_cast<void*>(index), n).b;       // read only from here on
    const int mi = (int)m, nruns = (mi + kKnnBox - 1) / kKnnBox, nbox = ((int)n + kKnnBox - 1) / kKnnBox;
    const int rc = knn_sort_into_boxes(mi, queries, q.sort, q.runs, s);
    if (rc != OGS_OK) return rc;
    OGS_LAUNCH(knn_start_kernel, dim3((unsigned)((nruns + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, mi, nruns, nbox, q.runs.sx,
               q.runs.sy, q.runs.sz, r.frame, r.first_key, q.start);
    OGS_LAUNCH_CHECK(0, s);
    return knn_launch_search(nruns, nbox, K, 0, q.runs, q.start, r, idx, d2, s);
}

}  // extern "C"
