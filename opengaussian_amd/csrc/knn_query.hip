// Exact K nearest neighbours BETWEEN TWO point sets: a persistent index of the reference set, queried many times
// (include/ogs_knn.h: ogs_knn_index_build, ogs_knn_query).
//
// ogs_knn_index_build is knn_sort_into_boxes (knn_boxes.h, which describes the sorted set and the walk over it) run on the
// reference set and kept, KEYED: besides what a walk reads, the Morton key of every box's first point and the bounding box that
// made the keys (the reference's FRAME).  A copy: `points` is not read again.
//
// ogs_knn_query:
//   1. GROUPING (knn_sort_queries, shared with ogs_knn_radius_count).  The same sort on the queries, keyed in the queries' OWN
//      bounding box: runs of 64 consecutive sorted queries are spatially coherent wherever the queries lie -- keyed in the
//      reference's frame, every query outside it would collapse into a boundary cell and a run would span the whole outside.
//   2. START BOX.  Per run, its median query (the middle of the run in sorted order) is keyed in the REFERENCE's frame (clamped
//      to its boundary cells when outside) and located among the per-box first keys by bisection: the last box whose first key
//      is not above it, clamped to [0, nbox).  One thread per run, at most 32 steps.  (The centre of the run's bounds was the
//      first choice and measured slower: a run that straddles a jump of the Morton curve has its centre far from both halves.)
//   3. SEARCH.  knn_search_kernel (knn_search.hip) from those start boxes; the result does not depend on them.
//
// No read-back, no float atomics, nothing waits on another workgroup.
#include "knn_boxes.h"
#include "../../include/ogs_knn.h"

namespace ogs {
namespace {

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

}  // namespace

int knn_sort_queries(int64_t n, const void* index, int64_t m, const float* queries, void* tmp, size_t tmp_bytes, const char* name,
                     bool with_start, hipStream_t s, KnnTwoSets& out) {
    Carver c(tmp);
    const SortedTmp q = SortedTmp::carve(c, m, with_start);
    if (tmp_bytes < q.bytes) {
        set_error("%s: tmp has %zu bytes, %zu needed (ogs_%s_tmp_bytes)", name, tmp_bytes, q.bytes, name);
        return OGS_ERR_INVALID_ARG;
    }
    out.q = q.boxes;
    out.start = q.start;
    out.r = IndexLayout::carve(const_cast<void*>(index), n).b;     // read only from here on
    out.nruns = (int)knn_nbox(m);
    out.nbox = (int)knn_nbox(n);
    return knn_sort_into_boxes((int)m, queries, q.sort, q.boxes, s);
}

}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_knn_index_bytes(int64_t n) {
    if (n <= 0 || !knn_size_ok(n)) return 0;
    return IndexLayout::carve(nullptr, n).bytes;
}

size_t ogs_knn_index_build_tmp_bytes(int64_t n) {
    if (n <= 0 || !knn_size_ok(n)) return 0;
    Carver c(nullptr);
    return SortTmp::carve(c, n).bytes;
}

int ogs_knn_index_build(int64_t n, const float* points, void* index, size_t index_bytes, void* tmp, size_t tmp_bytes,
                        void* stream_) {
    if (!knn_size_ok(n)) {
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
    if (n <= 0 || m <= 0 || !knn_size_ok(n) || !knn_size_ok(m)) return 0;
    Carver c(nullptr);
    return SortedTmp::carve(c, m, true).bytes;
}

int ogs_knn_query(int64_t n, const void* index, int64_t m, const float* queries, int32_t K, int32_t* idx, float* d2, void* tmp,
                  size_t tmp_bytes, void* stream_) {
    if (!knn_size_ok(n) || !knn_size_ok(m) || K < 1 || K > kKnnMaxK || m * (int64_t)K >= ((int64_t)1 << 31)) {
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
    KnnTwoSets w;
    const int rc = knn_sort_queries(n, index, m, queries, tmp, tmp_bytes, "knn_query", true, s, w);
    if (rc != OGS_OK) return rc;
    OGS_LAUNCH(knn_start_kernel, dim3((unsigned)((w.nruns + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, (int)m, w.nruns, w.nbox, w.q.sx,
               w.q.sy, w.q.sz, w.r.frame, w.r.first_key, w.start);
    OGS_LAUNCH_CHECK(0, s);
    return knn_launch_search(w.nruns, w.nbox, K, 0, w.q, w.start, w.r, idx, d2, s);
}

}  // extern "C"
