// The kNN graph backwards (include/ogs_knn.h): reverse-edge lists of an index table, the gather-sum over them (the adjoint of
// ogs_knn_aggregate), the per-edge dots (its gradient with respect to the weights) and the fused neighbour-smoothness energy
// with its gradient.  No float atomics, no kernel waits on another workgroup, nothing is read back to the host: every launch is
// sized from host-known bounds and every count that depends on the data stays in device memory.
//
// ogs_knn_transpose: key = idx (a value outside [0, R) becomes kDropKey), value = the flat slot number e = i * K + k; the
//   three-launch stable radix passes of radix_sort.hip, ceil(bits(R - 1) / 8) of them, the first one dropping the invalid slots.
//   A stable sort of ascending values by key leaves every row's slots ascending, so the result is unique.  begin[r] is the
//   lower bound of r in the sorted keys (a binary search per row: a row without an incoming edge gets begin[r] == begin[r + 1]
//   with no fill loop whose length depends on the data).
//
// The in-list walks (ogs_knn_aggregate_t, ogs_knn_smoothness_bwd) share one kernel body, graph_rows_kernel.  A row whose list
//   has at most kChunk slots is summed by the thread that owns the element: one fmaf chain from +0, slots ascending.  A longer
//   list is SPLIT: chunk c = slots [c * kChunk, (c + 1) * kChunk) of the list is one entry of a work list (row, chunk) built on
//   the device -- chunks per split row, exclusive scan, one fill -- and summed by a thread of its own into a partial row; a
//   further, small launch adds the partials of every split row in chunk order.  The
//   work list holds the split rows only (at most 2 * n * K / kChunk entries, a host-known bound), so a graph without a hub pays
//   one pass over begin[] for it and reads no indirection.
//
// Everything read from begin[] and slots[] is clamped or skipped before it addresses anything: begin values to [0, n * K], a
// pair with begin[r + 1] < begin[r] is an empty list, a slot outside [0, n * K) is skipped, and a work-list position at or past
// the bound is not written and not read (only inconsistent begin[] can get there).
//
// Compiled with -ffp-contract=off: every fmaf here is explicit, so the summation orders in the header are what the code does.
#include "ogs_common.h"
#include "../../include/ogs_knn.h"

#include <limits.h>

namespace ogs {
namespace {

constexpr int kChunk = 256;                             // slots of an in-list one work item sums
constexpr int kSumBlocks = 1024;                        // most workgroups (and partial records) of the energy total's first stage

// ---- reverse-edge lists -------------------------------------------------------------------------------------------------------
struct TransposeTmp {
    uint32_t* keys[2];                                  // [E] ping-pong
    uint32_t* vals;                                     // [E] the ping of the values; the pong is the caller's `slots`
    uint32_t* kept;                                     // [1] slots with 0 <= idx < R
    void* sort_tmp;
    size_t bytes;
    static TransposeTmp carve(void* p, int64_t E) {
        Carver c(p);
        TransposeTmp t{};
        t.keys[0] = c.take<uint32_t>((size_t)E);
        t.keys[1] = c.take<uint32_t>((size_t)E);
        t.vals = c.take<uint32_t>((size_t)E);
        t.kept = c.take<uint32_t>(1);
        t.sort_tmp = c.take<char>(sort_tmp_bytes(E));
        t.bytes = c.off;
        return t;
    }
};

__global__ __launch_bounds__(kBlock) void graph_keys_kernel(int64_t E, int64_t R, const int32_t* __restrict__ idx,
                                                            uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    const int j = idx[e];
    keys[e] = (j >= 0 && (int64_t)j < R) ? (uint32_t)j : kDropKey;       // R <= INT32_MAX: a valid key is never the drop key
    vals[e] = (uint32_t)e;
}

// begin[r] = sorted keys below r, r in [0, R]; the keys are the `*kept` valid ones, all below R
__global__ __launch_bounds__(kBlock) void graph_begin_kernel(int64_t R, int64_t E, const uint32_t* __restrict__ keys,
                                                             const uint32_t* __restrict__ kept, int32_t* __restrict__ begin) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r > R) return;
    const int64_t m = min((int64_t)*kept, E);
    int64_t lo = 0, hi = m;                             // first position whose key is >= r
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)keys[mid] < r) lo = mid + 1; else hi = mid;
    }
    begin[r] = (int32_t)lo;
}

// ---- in-lists -------------------------------------------------------------------------------------------------------------------
// the list of row r as positions [b, e) of slots[], whatever begin[] holds
__device__ __forceinline__ void list_range(const int32_t* __restrict__ begin, int64_t r, int64_t E, int64_t& b, int64_t& e) {
    b = min(max((int64_t)begin[r], (int64_t)0), E);
    e = min(max((int64_t)begin[r + 1], (int64_t)0), E);
    if (e < b) e = b;
}
__device__ __forceinline__ uint32_t chunks_of(int64_t deg) { return (uint32_t)((deg + kChunk - 1) / kChunk); }

struct ListsTmp {
    uint32_t* pcnt;                                     // [R] chunks of a split row, 0 for the others
    uint32_t* poff;                                     // [R] their exclusive prefix: first work-list entry of the row
    uint32_t* ptotal;                                   // [1] entries of the work list
    int32_t* item_row;                                  // [cap] row of every entry; its chunk is entry - poff[row]
    float* partial;                                     // [cap, D]
    void* scan_tmp;
    int64_t cap;
    size_t bytes;
    static int64_t capacity(int64_t E) { return 2 * (E / kChunk) + 1; }   // a split row has deg > kChunk: ceil(deg / kChunk) < 2 deg / kChunk
    static ListsTmp carve(void* p, int64_t E, int64_t R, int64_t D) {
        Carver c(p);
        ListsTmp t{};
        t.cap = capacity(E);
        t.pcnt = c.take<uint32_t>((size_t)R);
        t.poff = c.take<uint32_t>((size_t)R);
        t.ptotal = c.take<uint32_t>(1);
        t.item_row = c.take<int32_t>((size_t)t.cap);
        t.partial = c.take<float>((size_t)t.cap * (size_t)D);
        t.scan_tmp = c.take<char>(scan_tmp_bytes(R));
        t.bytes = c.off;
        return t;
    }
};

__global__ __launch_bounds__(kBlock) void graph_chunks_kernel(int64_t R, int64_t E, const int32_t* __restrict__ begin,
                                                              uint32_t* __restrict__ pcnt) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= R) return;
    int64_t b, e;
    list_range(begin, r, E, b, e);
    pcnt[r] = e - b > kChunk ? chunks_of(e - b) : 0u;
}

__global__ __launch_bounds__(kBlock) void graph_items_kernel(int64_t R, int64_t E, int64_t cap, const int32_t* __restrict__ begin,
                                                             const uint32_t* __restrict__ poff, int32_t* __restrict__ item_row) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= R) return;
    int64_t b, e;
    list_range(begin, r, E, b, e);
    if (e - b <= kChunk) return;
    const int64_t t0 = poff[r], t1 = min(t0 + (int64_t)chunks_of(e - b), cap);
    for (int64_t t = t0; t < t1; ++t) item_row[t] = (int32_t)r;
}

// What a walk adds per slot.  SMOOTH = false (ogs_knn_aggregate_t): w[s] * A[s / K, c].  SMOOTH = true (ogs_knn_smoothness_bwd):
// w[s] * (A[row, c] - A[s / K, c]), A = F.
template <int V, bool SMOOTH>
__device__ __forceinline__ void walk_slots(const int32_t* __restrict__ slots, const float* __restrict__ w, const float* __restrict__ A,
                                           int64_t E, int K, size_t D, size_t col, int64_t p0, int64_t p1, const float (&own)[V],
                                           float (&acc)[V]) {
#pragma unroll 4
    for (int64_t p = p0; p < p1; ++p) {
        const int s = slots[p];
        if (s < 0 || (int64_t)s >= E) continue;
        const float wv = w[s];
        const float* ar = A + (size_t)(s / K) * D + col;
        float x[V];
        if constexpr (V == 4) {
            const float4 v = *reinterpret_cast<const float4*>(ar);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
            x[0] = ar[0];
        }
#pragma unroll
        for (int u = 0; u < V; ++u) acc[u] = fmaf(wv, SMOOTH ? own[u] - x[u] : x[u], acc[u]);
    }
}

// the out-half of the smoothness gradient: acc = fmaf(w[i, k], F[i, c] - F[idx[i, k], c], acc), k ascending, valid slots only
template <int V>
__device__ __forceinline__ void walk_out_edges(const int32_t* __restrict__ idx, const float* __restrict__ w, const float* __restrict__ F,
                                               int64_t n, int K, size_t D, size_t col, int64_t row, const float (&own)[V],
                                               float (&acc)[V]) {
    const int32_t* ir = idx + (size_t)row * K;
    const float* wr = w + (size_t)row * K;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        const int j = ir[k];
        if (j < 0 || (int64_t)j >= n) continue;
        const float wv = wr[k];
        const float* fr = F + (size_t)j * D + col;
        if constexpr (V == 4) {
            const float4 v = *reinterpret_cast<const float4*>(fr);
            acc[0] = fmaf(wv, own[0] - v.x, acc[0]); acc[1] = fmaf(wv, own[1] - v.y, acc[1]);
            acc[2] = fmaf(wv, own[2] - v.z, acc[2]); acc[3] = fmaf(wv, own[3] - v.w, acc[3]);
        } else {
            acc[0] = fmaf(wv, own[0] - fr[0], acc[0]);
        }
    }
}

template <int V>
__device__ __forceinline__ void load_cols(const float* __restrict__ p, float (&v)[V]) {
    if constexpr (V == 4) {
        const float4 x = *reinterpret_cast<const float4*>(p);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
        v[0] = p[0];
    }
}
template <int V>
__device__ __forceinline__ void store_cols(float* __restrict__ p, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}

struct RowsArgs {
    int64_t R, E, n;                                    // rows of out, slots, rows of A (SMOOTH: n == R)
    int K, cols;                                        // cols = D / V
    const int32_t *begin, *slots, *idx;                 // idx: SMOOTH only
    const float *w, *A, *scale;                         // scale: SMOOTH only, device scalar
    float* out;                                         // [R, D]
    const uint32_t *poff, *ptotal;
    const int32_t* item_row;
    float* partial;
    int64_t cap;
    int64_t row_threads;                                // R * cols
    int64_t entry_base;                                 // row_threads rounded up to whole workgroups: first thread of the work list
};

// Threads [0, R * cols): element (row, column group) of a row that is not split, written here.  Threads from entry_base on (the
// launch reserves cap * cols of them): (entry t, column group) of the work list, the chunk's sum from +0 into partial[t].
template <int V, bool SMOOTH>
__global__ __launch_bounds__(kBlock) void graph_rows_kernel(RowsArgs a) {
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t D = (size_t)a.cols * V;
    float own[V], acc[V];
#pragma unroll
    for (int u = 0; u < V; ++u) { own[u] = 0.f; acc[u] = 0.f; }
    if (tid < a.entry_base) {
        if (tid >= a.row_threads) return;
        const int64_t row = tid / a.cols;
        const size_t col = (size_t)(tid - row * a.cols) * V;
        int64_t b, e;
        list_range(a.begin, row, a.E, b, e);
        if (e - b > kChunk) return;                     // split: graph_fold_kernel writes the row
        if constexpr (SMOOTH) {
            load_cols<V>(a.A + (size_t)row * D + col, own);
            walk_out_edges<V>(a.idx, a.w, a.A, a.n, a.K, D, col, row, own, acc);
        }
        walk_slots<V, SMOOTH>(a.slots, a.w, a.A, a.E, a.K, D, col, b, e, own, acc);
        if constexpr (SMOOTH) {
            const float sc = 2.f * a.scale[0];
#pragma unroll
            for (int u = 0; u < V; ++u) acc[u] *= sc;
        }
        store_cols<V>(a.out + (size_t)row * D + col, acc);
        return;
    }
    const int64_t q = tid - a.entry_base;
    const int64_t t = q / a.cols;
    if (t >= min((int64_t)*a.ptotal, a.cap)) return;
    const size_t col = (size_t)(q - t * a.cols) * V;
    const int64_t row = min(max((int64_t)a.item_row[t], (int64_t)0), a.R - 1);
    int64_t b, e;
    list_range(a.begin, row, a.E, b, e);
    const int64_t c = t - (int64_t)a.poff[row];
    if (c >= 0 && c < (int64_t)chunks_of(e - b)) {      // always, unless begin[] contradicts itself
        if constexpr (SMOOTH) load_cols<V>(a.A + (size_t)row * D + col, own);
        walk_slots<V, SMOOTH>(a.slots, a.w, a.A, a.E, a.K, D, col, b + c * kChunk, min(b + (c + 1) * kChunk, e), own, acc);
    }
    store_cols<V>(a.partial + (size_t)t * D + col, acc);
}

// The thread of a split row's FIRST work-list entry adds the row's partials in chunk order, partial 0 first, and writes the row
// (SMOOTH: the out-half chain from +0 first, then the partials on top of it, then the scale).
template <int V, bool SMOOTH>
__global__ __launch_bounds__(kBlock) void graph_fold_kernel(RowsArgs a) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t t = q / a.cols;
    const int64_t total = min((int64_t)*a.ptotal, a.cap);
    if (t >= total) return;
    const size_t D = (size_t)a.cols * V, col = (size_t)(q - t * a.cols) * V;
    const int64_t row = min(max((int64_t)a.item_row[t], (int64_t)0), a.R - 1);
    if (t != (int64_t)a.poff[row]) return;
    int64_t b, e;
    list_range(a.begin, row, a.E, b, e);
    const int64_t t1 = min(t + (int64_t)chunks_of(e - b), total);
    float own[V], acc[V], p[V];
    if constexpr (SMOOTH) {
#pragma unroll
        for (int u = 0; u < V; ++u) acc[u] = 0.f;
        load_cols<V>(a.A + (size_t)row * D + col, own);
        walk_out_edges<V>(a.idx, a.w, a.A, a.n, a.K, D, col, row, own, acc);
        for (int64_t s = t; s < t1; ++s) {
            load_cols<V>(a.partial + (size_t)s * D + col, p);
#pragma unroll
            for (int u = 0; u < V; ++u) acc[u] += p[u];
        }
        const float sc = 2.f * a.scale[0];
#pragma unroll
        for (int u = 0; u < V; ++u) acc[u] *= sc;
    } else {
        load_cols<V>(a.partial + (size_t)t * D + col, acc);
        for (int64_t s = t + 1; s < t1; ++s) {
            load_cols<V>(a.partial + (size_t)s * D + col, p);
#pragma unroll
            for (int u = 0; u < V; ++u) acc[u] += p[u];
        }
    }
    store_cols<V>(a.out + (size_t)row * D + col, acc);
}

int64_t blocks_for(int64_t threads) { return (threads + kBlock - 1) / kBlock; }

// work list of the split rows, then the walk, then the fold
template <bool SMOOTH>
int launch_rows(RowsArgs a, int D, bool vec, void* tmp, hipStream_t s, const char* what) {
    const ListsTmp t = ListsTmp::carve(tmp, a.E, a.R, D);
    a.cols = vec ? D / 4 : D;
    a.poff = t.poff; a.ptotal = t.ptotal; a.item_row = t.item_row; a.partial = t.partial; a.cap = t.cap;
    a.row_threads = a.R * a.cols;
    const int64_t rb = blocks_for(a.R), fold_blocks = blocks_for(t.cap * a.cols);
    const int64_t blocks = blocks_for(a.row_threads) + fold_blocks;
    if (blocks > (int64_t)INT32_MAX) { set_error("%s: R * D = %lld too large", what, (long long)(a.R * D)); return OGS_ERR_INVALID_ARG; }
    OGS_LAUNCH(graph_chunks_kernel, dim3((unsigned)rb), dim3(kBlock), 0, s, a.R, a.E, a.begin, t.pcnt);
    OGS_LAUNCH_CHECK(0, s);
    const int rc = exclusive_scan_u32(t.pcnt, nullptr, t.poff, a.R, t.ptotal, t.scan_tmp, s, 0);
    if (rc != OGS_OK) return rc;
    OGS_LAUNCH(graph_items_kernel, dim3((unsigned)rb), dim3(kBlock), 0, s, a.R, a.E, t.cap, a.begin, (const uint32_t*)t.poff,
               t.item_row);
    OGS_LAUNCH_CHECK(0, s);
    a.entry_base = blocks_for(a.row_threads) * kBlock;  // the entry threads start at a workgroup boundary
    void (*rows)(RowsArgs) = vec ? graph_rows_kernel<4, SMOOTH> : graph_rows_kernel<1, SMOOTH>;
    void (*fold)(RowsArgs) = vec ? graph_fold_kernel<4, SMOOTH> : graph_fold_kernel<1, SMOOTH>;
    OGS_LAUNCH_NAMED(SMOOTH ? "graph_rows_kernel<smooth>" : "graph_rows_kernel", rows, dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
    OGS_LAUNCH_CHECK(0, s);
    OGS_LAUNCH_NAMED(SMOOTH ? "graph_fold_kernel<smooth>" : "graph_fold_kernel", fold, dim3((unsigned)fold_blocks), dim3(kBlock), 0, s, a);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

// ---- per-edge and per-row reductions over the columns ---------------------------------------------------------------------------
// A slot (or a row) is owned by a group of L consecutive lanes, L a power of two that depends on D alone: lane l of the group
// sums the columns l, l + L, l + 2 L, ... as one fmaf chain from +0, then the group folds by xor-shuffles with the masks
// L / 2, L / 4, ..., 1 (a + b on both sides of a pair: every lane ends with the same bits).
__host__ __device__ inline int lanes_for(int D) {
    int L = 1;
    while (L < kWave && L * 8 < D) L *= 2;
    return L;
}
__device__ __forceinline__ float group_fold(float v, int L) {
    for (int m = L >> 1; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// SQDIFF = false: gw = sum_c G[i, c] * X[j, c].  SQDIFF = true: gw = scale * sum_c (F[i, c] - F[j, c])^2 with G = X = F.
template <bool SQDIFF>
__global__ __launch_bounds__(kBlock) void graph_edges_kernel(int64_t E, int K, int64_t R, int D, int L, const int32_t* __restrict__ idx,
                                                             const float* __restrict__ G, const float* __restrict__ X,
                                                             const float* __restrict__ scale, float* __restrict__ gw) {
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t e = tid / L;                          // a group never straddles a wave: L divides kWave
    if (e >= E) return;
    const int l = (int)(tid - e * L);
    const int j = idx[e];
    const bool ok = j >= 0 && (int64_t)j < R;
    float acc = 0.f;
    if (ok) {
        const float* g = G + (size_t)(e / K) * D;
        const float* x = X + (size_t)j * D;
        for (int c = l; c < D; c += L) {
            if constexpr (SQDIFF) { const float d = g[c] - x[c]; acc = fmaf(d, d, acc); }
            else acc = fmaf(g[c], x[c], acc);
        }
    }
    acc = group_fold(acc, L);
    if (l == 0) gw[e] = ok ? (SQDIFF ? scale[0] * acc : acc) : 0.f;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}
// sum of (a, b) over the workgroup in a fixed order; valid in thread 0
__device__ __forceinline__ void block_sum2_d(double& a, double& b, double* red /* [2 * kBlock / kWave] */) {
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    const int w = threadIdx.x / kWave;
    if (lane_id() == 0) { red[2 * w] = a; red[2 * w + 1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = red[0]; b = red[1];
        for (int k = 1; k < kBlock / kWave; ++k) { a += red[2 * k]; b += red[2 * k + 1]; }
    }
}

// row energies: e[i] = the chain acc = fmaf(w[i, k], d2(i, k), acc) from +0, k ascending over the valid slots, d2 by the group
__global__ __launch_bounds__(kBlock) void graph_energy_kernel(int64_t n, int K, int D, int L, const int32_t* __restrict__ idx,
                                                              const float* __restrict__ w, const float* __restrict__ F,
                                                              float* __restrict__ energy, int32_t* __restrict__ valid) {
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t i = tid / L;
    if (i >= n) return;
    const int l = (int)(tid - i * L);
    const float* fi = F + (size_t)i * D;
    float acc = 0.f;
    int cnt = 0;
    for (int k = 0; k < K; ++k) {
        const int j = idx[(size_t)i * K + k];
        if (j < 0 || (int64_t)j >= n) continue;         // the same for every lane of the group
        const float* fj = F + (size_t)j * D;
        float d2 = 0.f;
        for (int c = l; c < D; c += L) { const float d = fi[c] - fj[c]; d2 = fmaf(d, d, d2); }
        d2 = group_fold(d2, L);
        acc = fmaf(w[(size_t)i * K + k], d2, acc);
        ++cnt;
    }
    if (l == 0) { energy[i] = acc; valid[i] = cnt; }
}

// the total in two stages, both in a fixed order: grid-stride fp64 partial sums per workgroup, then one workgroup over them
__global__ __launch_bounds__(kBlock) void graph_energy_partials_kernel(int64_t n, const float* __restrict__ energy,
                                                                       const int32_t* __restrict__ valid, double2* __restrict__ partials) {
    __shared__ double red[2 * kBlock / kWave];
    double a = 0.0, b = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        a += (double)energy[i];
        b += (double)valid[i];
    }
    block_sum2_d(a, b, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = make_double2(a, b);
}
__global__ __launch_bounds__(kBlock) void graph_energy_total_kernel(int nparts, const double2* __restrict__ partials,
                                                                    double* __restrict__ total) {
    __shared__ double red[2 * kBlock / kWave];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nparts; i += kBlock) { const double2 p = partials[i]; a += p.x; b += p.y; }
    block_sum2_d(a, b, red);
    if (threadIdx.x == 0) { total[0] = a; total[1] = b; }
}

struct EnergyTmp {
    int32_t* valid;                                     // [n] valid slots of every row
    double2* partials;                                  // [kSumBlocks]
    size_t bytes;
    static EnergyTmp carve(void* p, int64_t n) {
        Carver c(p);
        EnergyTmp t{};
        t.valid = c.take<int32_t>((size_t)n);
        t.partials = c.take<double2>(kSumBlocks);
        t.bytes = c.off;
        return t;
    }
};

bool graph_sizes_ok(int64_t n, int32_t K, int64_t R) {
    return n >= 0 && K >= 0 && R >= 0 && R <= (int64_t)INT32_MAX && n * (int64_t)K < ((int64_t)1 << 31);
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_knn_transpose_chunk(void) { return kChunk; }

size_t ogs_knn_transpose_tmp_bytes(int64_t n, int32_t K, int64_t R) {
    if (!graph_sizes_ok(n, K, R) || n * (int64_t)K == 0) return 0;
    return TransposeTmp::carve(nullptr, n * (int64_t)K).bytes;
}

int ogs_knn_transpose(int64_t n, int32_t K, int64_t R, const int32_t* idx, int32_t* begin, int32_t* slots, void* tmp,
                      size_t tmp_bytes, void* stream_) {
    if (!graph_sizes_ok(n, K, R)) {
        set_error("knn_transpose: bad sizes (n=%lld K=%d R=%lld; n * K < 2^31, 0 <= R <= INT32_MAX)", (long long)n, K, (long long)R);
        return OGS_ERR_INVALID_ARG;
    }
    if (!begin) { set_error("knn_transpose: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int64_t E = n * (int64_t)K;
    if (E == 0 || R == 0) {                             // no slot can be valid
        OGS_HIP_CHECK(hipMemsetAsync(begin, 0, (size_t)(R + 1) * sizeof(int32_t), s));
        return OGS_OK;
    }
    if (!idx || !slots || !tmp) { set_error("knn_transpose: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    const TransposeTmp t = TransposeTmp::carve(tmp, E);
    if (tmp_bytes < t.bytes) {
        set_error("knn_transpose: tmp has %zu bytes, %zu needed (ogs_knn_transpose_tmp_bytes)", tmp_bytes, t.bytes);
        return OGS_ERR_INVALID_ARG;
    }
    int key_bits = 1;
    while (key_bits < 31 && ((int64_t)1 << key_bits) < R) ++key_bits;        // keys are 0 .. R - 1
    const int npass = (key_bits + 7) / 8;
    // the invalid slots are dropped and t.kept is left holding the count; three-launch passes: nothing waits on another workgroup
    RadixSort sort = {{t.keys[0], t.keys[1]}, {}, E, nullptr, npass, {}, {}, true, t.kept, t.sort_tmp, RadixImpl::ThreeLaunch};
    sort.vals[npass & 1] = reinterpret_cast<uint32_t*>(slots);       // the last pass writes into `slots`
    sort.vals[(npass & 1) ^ 1] = t.vals;
    for (int pass = 0; pass < npass; ++pass) {
        sort.shift[pass] = 8 * pass;
        sort.bits[pass] = min(8, key_bits - 8 * pass);
    }
    OGS_LAUNCH(graph_keys_kernel, dim3((unsigned)blocks_for(E)), dim3(kBlock), 0, s, E, R, idx, t.keys[0], sort.vals[0]);
    OGS_LAUNCH_CHECK(0, s);
    const int rc = radix_sort(sort, s, 0);
    if (rc != OGS_OK) return rc;
    OGS_LAUNCH(graph_begin_kernel, dim3((unsigned)blocks_for(R + 1)), dim3(kBlock), 0, s, R, E, (const uint32_t*)t.keys[npass & 1],
               (const uint32_t*)t.kept, begin);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

size_t ogs_knn_aggregate_t_tmp_bytes(int64_t n, int32_t K, int64_t R, int32_t D) {
    if (!graph_sizes_ok(n, K, R) || D < 1 || R == 0) return 0;
    return ListsTmp::carve(nullptr, n * (int64_t)K, R, D).bytes;
}

int ogs_knn_aggregate_t(int64_t n, int32_t K, int64_t R, int32_t D, const int32_t* begin, const int32_t* slots, const float* w,
                        const float* G, float* out, void* tmp, size_t tmp_bytes, void* stream_) {
    if (!graph_sizes_ok(n, K, R) || D < 1) {
        set_error("knn_aggregate_t: bad sizes (n=%lld K=%d R=%lld D=%d)", (long long)n, K, (long long)R, D);
        return OGS_ERR_INVALID_ARG;
    }
    if (R == 0) return OGS_OK;
    const int64_t E = n * (int64_t)K;
    if (!begin || !out || !tmp || (E > 0 && (!slots || !w || !G))) { set_error("knn_aggregate_t: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    const size_t need = ListsTmp::carve(nullptr, E, R, D).bytes;
    if (tmp_bytes < need) {
        set_error("knn_aggregate_t: tmp has %zu bytes, %zu needed (ogs_knn_aggregate_t_tmp_bytes)", tmp_bytes, need);
        return OGS_ERR_INVALID_ARG;
    }
    RowsArgs a{};
    a.R = R; a.E = E; a.n = n; a.K = K;
    a.begin = begin; a.slots = slots; a.w = w; a.A = G; a.out = out;
    const bool vec = D % 4 == 0 && aligned16(G) && aligned16(out) && aligned16(tmp);      // tmp: the partial rows
    return launch_rows<false>(a, D, vec, tmp, static_cast<hipStream_t>(stream_), "knn_aggregate_t");
}

int ogs_knn_edge_dots(int64_t n, int32_t K, int64_t R, int32_t D, const int32_t* idx, const float* G, const float* X, float* gw,
                      void* stream_) {
    if (!graph_sizes_ok(n, K, R) || D < 1) {
        set_error("knn_edge_dots: bad sizes (n=%lld K=%d R=%lld D=%d)", (long long)n, K, (long long)R, D);
        return OGS_ERR_INVALID_ARG;
    }
    const int64_t E = n * (int64_t)K;
    if (E == 0) return OGS_OK;
    if (!idx || !G || !gw || (R > 0 && !X)) { set_error("knn_edge_dots: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int L = lanes_for(D);
    OGS_LAUNCH(graph_edges_kernel<false>, dim3((unsigned)blocks_for(E * L)), dim3(kBlock), 0, s, E, K, R, D, L, idx, G, X,
               (const float*)nullptr, gw);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

size_t ogs_knn_smoothness_fwd_tmp_bytes(int64_t n) {
    if (n <= 0 || n > (int64_t)INT32_MAX) return 0;
    return EnergyTmp::carve(nullptr, n).bytes;
}

int ogs_knn_smoothness_fwd(int64_t n, int32_t K, int32_t D, const int32_t* idx, const float* w, const float* F, float* energy,
                           double* total, void* tmp, size_t tmp_bytes, void* stream_) {
    if (!graph_sizes_ok(n, K, n) || D < 1) {
        set_error("knn_smoothness_fwd: bad sizes (n=%lld K=%d D=%d)", (long long)n, K, D);
        return OGS_ERR_INVALID_ARG;
    }
    if (!total) { set_error("knn_smoothness_fwd: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (n == 0) {
        OGS_HIP_CHECK(hipMemsetAsync(total, 0, 2 * sizeof(double), s));
        return OGS_OK;
    }
    if (!energy || !F || !tmp || (K > 0 && (!idx || !w))) { set_error("knn_smoothness_fwd: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    const EnergyTmp t = EnergyTmp::carve(tmp, n);
    if (tmp_bytes < t.bytes) {
        set_error("knn_smoothness_fwd: tmp has %zu bytes, %zu needed (ogs_knn_smoothness_fwd_tmp_bytes)", tmp_bytes, t.bytes);
        return OGS_ERR_INVALID_ARG;
    }
    const int L = lanes_for(D);
    OGS_LAUNCH(graph_energy_kernel, dim3((unsigned)blocks_for(n * L)), dim3(kBlock), 0, s, n, K, D, L, idx, w, F, energy, t.valid);
    OGS_LAUNCH_CHECK(0, s);
    const int nparts = (int)min((int64_t)kSumBlocks, blocks_for(n));
    OGS_LAUNCH(graph_energy_partials_kernel, dim3((unsigned)nparts), dim3(kBlock), 0, s, n, (const float*)energy,
               (const int32_t*)t.valid, t.partials);
    OGS_LAUNCH_CHECK(0, s);
    OGS_LAUNCH(graph_energy_total_kernel, dim3(1), dim3(kBlock), 0, s, nparts, (const double2*)t.partials, total);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

size_t ogs_knn_smoothness_bwd_tmp_bytes(int64_t n, int32_t K, int32_t D) { return ogs_knn_aggregate_t_tmp_bytes(n, K, n, D); }

int ogs_knn_smoothness_bwd(int64_t n, int32_t K, int32_t D, const int32_t* idx, const float* w, const float* F, const int32_t* begin,
                           const int32_t* slots, const float* scale, float* gF, float* gw, void* tmp, size_t tmp_bytes,
                           void* stream_) {
    if (!graph_sizes_ok(n, K, n) || D < 1) {
        set_error("knn_smoothness_bwd: bad sizes (n=%lld K=%d D=%d)", (long long)n, K, D);
        return OGS_ERR_INVALID_ARG;
    }
    if (n == 0) return OGS_OK;
    const int64_t E = n * (int64_t)K;
    if (!F || !begin || !scale || !gF || !tmp || (E > 0 && (!idx || !w || !slots))) {
        set_error("knn_smoothness_bwd: NULL pointer");
        return OGS_ERR_INVALID_ARG;
    }
    const size_t need = ListsTmp::carve(nullptr, E, n, D).bytes;
    if (tmp_bytes < need) {
        set_error("knn_smoothness_bwd: tmp has %zu bytes, %zu needed (ogs_knn_smoothness_bwd_tmp_bytes)", tmp_bytes, need);
        return OGS_ERR_INVALID_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    RowsArgs a{};
    a.R = n; a.E = E; a.n = n; a.K = K;
    a.begin = begin; a.slots = slots; a.idx = idx; a.w = w; a.A = F; a.scale = scale; a.out = gF;
    const bool vec = D % 4 == 0 && aligned16(F) && aligned16(gF) && aligned16(tmp);
    const int rc = launch_rows<true>(a, D, vec, tmp, s, "knn_smoothness_bwd");
    if (rc != OGS_OK || !gw || E == 0) return rc;
    const int L = lanes_for(D);
    OGS_LAUNCH(graph_edges_kernel<true>, dim3((unsigned)blocks_for(E * L)), dim3(kBlock), 0, s, E, K, n, D, L, idx, F, F, scale, gw);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

}  // extern "C"
