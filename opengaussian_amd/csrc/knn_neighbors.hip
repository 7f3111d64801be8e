// Exact K nearest neighbours WITH indices at scene scale, and the fixed-degree gather-sum over them (include/ogs_knn.h).
//
// ogs_knn_neighbors: sort once, search in boxes.  This file holds the sort -- knn_sort_into_boxes, the front half every search
// over sorted boxes begins with (knn_boxes.h describes the sorted set and the walk over it):
//   1. bounding box of the cloud (two stages: per-workgroup partials, folded again by every workgroup of the key kernel),
//   2. a 30-bit Morton key per point (10 bits per axis, every cell clamped to [0, 1023] whatever the coordinate is),
//   3. (key, id) sorted by four stable radix passes (radix_sort.hip; the three-launch passes: nothing waits on another workgroup),
//   4. the coordinates gathered into sorted order, coordinate-wise, and the axis-aligned bounds of every box.
// The search itself is knn_search_kernel (knn_search.hip), here with the set against itself: a run of queries IS a box, and its walk
// starts there.
//
// ogs_knn_aggregate: out[i, c] = sum_k w[i, k] * X[idx[i, k], c] as one fmaf chain per element, k ascending, one thread per
// output element (per four columns where D and the bases allow 16-byte accesses); no [n, K, D] buffer, no atomics.
//
// This file is compiled with -ffp-contract=off: every fmaf of the aggregate is written out, and nothing else here may become one.
#include "knn_boxes.h"
#include "../../include/ogs_knn.h"

namespace ogs {
namespace {

// min / max of six values over the workgroup; every thread returns with the result.  fminf / fmaxf drop NaNs.
__device__ __forceinline__ void block_bounds(float (&lo)[3], float (&hi)[3], float (*sh)[6]) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = wave_min_f(lo[a]); hi[a] = wave_max_f(hi[a]); }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { sh[wave][a] = lo[a]; sh[wave][3 + a] = hi[a]; }
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = sh[0][a]; hi[a] = sh[0][3 + a];
#pragma unroll
        for (int w = 1; w < kBlock / kWave; ++w) { lo[a] = fminf(lo[a], sh[w][a]); hi[a] = fmaxf(hi[a], sh[w][3 + a]); }
    }
}

__global__ __launch_bounds__(kBlock) void knn_bounds_kernel(int n, const float* __restrict__ pts, float* __restrict__ partial) {
    __shared__ float sh[kBlock / kWave][6];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = pts[(size_t)i * 3 + a];
            lo[a] = fminf(lo[a], v); hi[a] = fmaxf(hi[a], v);
        }
    }
    block_bounds(lo, hi, sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { partial[blockIdx.x * 6 + a] = lo[a]; partial[blockIdx.x * 6 + 3 + a] = hi[a]; }
    }
}

// frame (may be nullptr): the folded bounds, min xyz then max xyz, written by the first workgroup
__global__ __launch_bounds__(kBlock) void knn_keys_kernel(int n, const float* __restrict__ pts, const float* __restrict__ partial,
                                                          int nparts, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                          float* __restrict__ frame) {
    __shared__ float sh[kBlock / kWave][6];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if ((int)threadIdx.x < nparts) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = partial[threadIdx.x * 6 + a]; hi[a] = partial[threadIdx.x * 6 + 3 + a]; }
    }
    block_bounds(lo, hi, sh);
    if (frame && blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { frame[a] = lo[a]; frame[3 + a] = hi[a]; }
    }
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {pts[(size_t)i * 3], pts[(size_t)i * 3 + 1], pts[(size_t)i * 3 + 2]};
    keys[i] = knn_morton(p, lo, hi);
    vals[i] = (uint32_t)i;
}

// one wave per box: gather its points into sorted order and fold their bounds; first_key (may be nullptr) takes the sorted key
// of the box's first point
__global__ __launch_bounds__(kBlock) void knn_gather_kernel(int n, int nbox, const float* __restrict__ pts,
                                                            const uint32_t* __restrict__ order,
                                                            const uint32_t* __restrict__ sorted_keys, float* __restrict__ sx,
                                                            float* __restrict__ sy, float* __restrict__ sz,
                                                            int32_t* __restrict__ sid, float* __restrict__ box,
                                                            uint32_t* __restrict__ first_key) {
    const int lane = threadIdx.x & (kWave - 1);
    const int b = blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (b >= nbox) return;
    const int64_t p = (int64_t)b * kKnnBox + lane;
    float x = __builtin_nanf(""), y = x, z = x;
    int id = kNoId;
    if (p < n) {
        id = (int)min(order[p], (uint32_t)(n - 1));                // a permutation of [0, n); clamped before it addresses anything
        x = pts[(size_t)id * 3]; y = pts[(size_t)id * 3 + 1]; z = pts[(size_t)id * 3 + 2];
    }
    sx[p] = x; sy[p] = y; sz[p] = z; sid[p] = id;
    const float v[6] = {wave_min_f(x), wave_min_f(y), wave_min_f(z), wave_max_f(x), wave_max_f(y), wave_max_f(z)};
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 6; ++a) box[(size_t)a * nbox + b] = v[a];
        if (first_key) first_key[b] = sorted_keys[(size_t)b * kKnnBox];      // b * kKnnBox < n: the box has a point
    }
}

// ---- the gather-sum ---------------------------------------------------------------------------------------------------------
// V = 4: D is a multiple of 4 and X / out are 16-byte aligned; a thread owns four columns of one row.
template <int V>
__global__ __launch_bounds__(kBlock) void knn_aggregate_kernel(int64_t total, int K, int64_t R, int cols,
                                                               const int32_t* __restrict__ idx, const float* __restrict__ w,
                                                               const float* __restrict__ X, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // element (row, column group)
    if (e >= total) return;
    const int64_t row = e / cols;
    const int c = (int)(e - row * cols);
    const size_t D = (size_t)cols * V;
    const int32_t* ir = idx + (size_t)row * K;
    const float* wr = w + (size_t)row * K;
    float acc[V];
#pragma unroll
    for (int u = 0; u < V; ++u) acc[u] = 0.f;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        const int j = ir[k];
        if (j < 0 || (int64_t)j >= R) continue;                    // an empty or foreign slot: its weight is not looked at
        const float wv = wr[k];
        const float* xr = X + (size_t)j * D + (size_t)c * V;
        if constexpr (V == 4) {
            const float4 x = *reinterpret_cast<const float4*>(xr);
            acc[0] = fmaf(wv, x.x, acc[0]); acc[1] = fmaf(wv, x.y, acc[1]);
            acc[2] = fmaf(wv, x.z, acc[2]); acc[3] = fmaf(wv, x.w, acc[3]);
        } else {
            acc[0] = fmaf(wv, xr[0], acc[0]);
        }
    }
    float* orow = out + (size_t)row * D + (size_t)c * V;
    if constexpr (V == 4) *reinterpret_cast<float4*>(orow) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    else orow[0] = acc[0];
}

}  // namespace

int knn_sort_into_boxes(int n, const float* pts, const KnnSortScratch& t, const KnnBoxes& out, hipStream_t s) {
    const int nbox = (int)knn_nbox(n);
    const int nparts = min(kBoundBlocks, (n + kBlock - 1) / kBlock);
    OGS_LAUNCH(knn_bounds_kernel, dim3((unsigned)nparts), dim3(kBlock), 0, s, n, pts, t.partial);
    OGS_LAUNCH_CHECK(0, s);
    OGS_LAUNCH(knn_keys_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, n, pts, t.partial, nparts,
               t.keys[0], t.vals[0], out.frame);
    OGS_LAUNCH_CHECK(0, s);
    // 30 key bits; an even number of passes ends in [0]
    const RadixSort sort = {{t.keys[0], t.keys[1]}, {t.vals[0], t.vals[1]}, n, nullptr, 4, {0, 8, 16, 24}, {8, 8, 8, 6},
                            false, nullptr, t.sort_tmp, RadixImpl::ThreeLaunch};
    const int rc = radix_sort(sort, s, 0);
    if (rc != OGS_OK) return rc;
    const int wpb = kBlock / kWave;
    OGS_LAUNCH(knn_gather_kernel, dim3((unsigned)((nbox + wpb - 1) / wpb)), dim3(kBlock), 0, s, n, nbox, pts, t.vals[0], t.keys[0],
               out.sx, out.sy, out.sz, out.sid, out.box, out.first_key);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_knn_box_points(void) { return kKnnBox; }
size_t ogs_knn_max_k(void) { return kKnnMaxK; }

size_t ogs_knn_neighbors_tmp_bytes(int64_t n) {
    if (n <= 0 || !knn_size_ok(n)) return 0;
    Carver c(nullptr);
    return SortedTmp::carve(c, n).bytes;
}

int ogs_knn_neighbors(int64_t n, const float* points, int32_t K, int32_t exclude_self, int32_t* idx, float* d2, void* tmp,
                      size_t tmp_bytes, void* stream_) {
    if (!knn_size_ok(n) || K < 1 || K > kKnnMaxK || n * (int64_t)K >= ((int64_t)1 << 31)) {
        set_error("knn_neighbors: bad sizes (n=%lld K=%d; 1 <= K <= %d, n * K < 2^31)", (long long)n, K, kKnnMaxK);
        return OGS_ERR_INVALID_ARG;
    }
    if (n == 0) return OGS_OK;
    if (!points || !idx || !d2 || !tmp) { set_error("knn_neighbors: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    Carver c(tmp);
    const SortedTmp t = SortedTmp::carve(c, n);                    // unkeyed: the search starts at the own box
    if (tmp_bytes < t.bytes) {
        set_error("knn_neighbors: tmp has %zu bytes, %zu needed (ogs_knn_neighbors_tmp_bytes)", tmp_bytes, t.bytes);
        return OGS_ERR_INVALID_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int ni = (int)n, nbox = (int)knn_nbox(n);
    const int rc = knn_sort_into_boxes(ni, points, t.sort, t.boxes, s);
    if (rc != OGS_OK) return rc;
    return knn_launch_search(nbox, nbox, K, exclude_self ? 1 : 0, t.boxes, nullptr, t.boxes, idx, d2, s);
}

int ogs_knn_aggregate(int64_t n, int32_t K, int64_t R, int32_t D, const int32_t* idx, const float* w, const float* X, float* out,
                      void* stream_) {
    if (n < 0 || K < 0 || R < 0 || D < 1) {
        set_error("knn_aggregate: bad sizes (n=%lld K=%d R=%lld D=%d)", (long long)n, K, (long long)R, D);
        return OGS_ERR_INVALID_ARG;
    }
    if (n == 0) return OGS_OK;
    if (!out || (K > 0 && (!idx || !w)) || (K > 0 && R > 0 && !X)) { set_error("knn_aggregate: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const bool vec = D % 4 == 0 && ((uintptr_t)X & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const int cols = vec ? D / 4 : D;
    const int64_t total = n * cols, blocks = (total + kBlock - 1) / kBlock;
    if (blocks > (int64_t)INT32_MAX) { set_error("knn_aggregate: n * D = %lld too large", (long long)(n * D)); return OGS_ERR_INVALID_ARG; }
    if (vec) OGS_LAUNCH(knn_aggregate_kernel<4>, dim3((unsigned)blocks), dim3(kBlock), 0, s, total, K, R, cols, idx, w, X, out);
    else OGS_LAUNCH(knn_aggregate_kernel<1>, dim3((unsigned)blocks), dim3(kBlock), 0, s, total, K, R, cols, idx, w, X, out);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

}  // extern "C"
