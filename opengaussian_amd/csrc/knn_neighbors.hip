// Exact K nearest neighbours WITH indices at scene scale, and the fixed-degree gather-sum over them (include/ogs_knn.h).
//
// ogs_knn_neighbors: sort once, search in boxes.
//   1. bounding box of the cloud (two stages: per-workgroup partials, folded again by every workgroup of the key kernel),
//   2. a 30-bit Morton key per point (10 bits per axis, every cell clamped to [0, 1023] whatever the coordinate is),
//   3. (key, id) sorted by four stable radix passes (binning.hip; the three-launch passes: nothing waits on another workgroup),
//   4. the coordinates gathered into sorted order, coordinate-wise, and the axis-aligned bounds of every run of kKnnBox = 64
//      consecutive sorted points (a BOX),
//   5. the search: one wave owns one box of queries, one query per lane.  A lane keeps its K best (d2, id) pairs in registers
//      as a sorted list (templated on 4 / 8 / 16 / 32; a requested K rounds up and the first K pairs are stored).  Candidate
//      boxes are visited outward from the own box in sorted order: 64 candidates at a time, one per lane, are tested against
//      the own box's bounds, and a box is skipped when its lower bound is STRICTLY above the largest K-th d2 of the wave's
//      queries (an equal distance with a smaller id still displaces).  The lower bound is the d2 expression itself on the
//      per-axis gaps max(lo_c - hi_q, lo_q - hi_c, 0): round-to-nearest subtraction, product and sum are monotone, so the
//      bound is <= the computed fp32 d2 of every pair of the two boxes and needs no safety margin.  A visited box is staged in
//      LDS coordinate by coordinate and read with broadcast 16-byte reads, four points of one coordinate at a time.
//      A cloud that cannot be pruned (all points coincident: every bound and every K-th value is 0) visits every box: one brute
//      pass of n^2 pairs, still correct.
//   The order (d2, id) is total, so the result is unique and does not depend on the order of visits.
//
// ogs_knn_aggregate: out[i, c] = sum_k w[i, k] * X[idx[i, k], c] as one fmaf chain per element, k ascending, one thread per
// output element (per four columns where D and the bases allow 16-byte accesses); no [n, K, D] buffer, no atomics.
//
// This file is compiled with -ffp-contract=off: d2 = (dx*dx + dy*dy) + dz*dz, exactly so (the fmaf of the aggregate is explicit).
#include "ogs_common.h"
#include "../../include/ogs_knn.h"

#include <limits.h>

namespace ogs {
namespace {

constexpr int kKnnBox = kWave;                          // points per box = queries per wave = candidates per staging round
constexpr int kKnnMaxK = 32;
constexpr int kBoundBlocks = 256;                       // workgroups (and partial records) of the bounding-box pass
constexpr int kNoId = INT_MAX;                          // id of an empty list slot and of a padding point: above every real id
static_assert(kBoundBlocks <= kBlock, "one thread folds one partial record");

struct NeighborsTmp {
    float* partial;                                     // [kBoundBlocks][6] min xyz, max xyz
    uint32_t* keys[2];                                  // [n] Morton keys, ping-pong
    uint32_t* vals[2];                                  // [n] point ids, ping-pong; vals[0] holds the sorted order at the end
    float *sx, *sy, *sz;                                // [nbox * kKnnBox] sorted coordinates, NaN past n
    int32_t* sid;                                       // [nbox * kKnnBox] sorted ids (clamped to [0, n)), kNoId past n
    float* box;                                         // [6][nbox] min xyz, max xyz of every box
    void* sort_tmp;
    size_t bytes;
    static NeighborsTmp carve(void* p, int64_t n) {
        Carver c(p);
        NeighborsTmp t{};
        const size_t nbox = (size_t)((n + kKnnBox - 1) / kKnnBox), npad = nbox * kKnnBox;
        t.partial = c.take<float>((size_t)kBoundBlocks * 6);
        for (int i = 0; i < 2; ++i) { t.keys[i] = c.take<uint32_t>((size_t)n); t.vals[i] = c.take<uint32_t>((size_t)n); }
        t.sx = c.take<float>(npad); t.sy = c.take<float>(npad); t.sz = c.take<float>(npad);
        t.sid = c.take<int32_t>(npad);
        t.box = c.take<float>(6 * nbox);
        t.sort_tmp = c.take<char>(sort_tmp_bytes(n));
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

__global__ __launch_bounds__(kBlock) void knn_keys_kernel(int n, const float* __restrict__ pts, const float* __restrict__ partial,
                                                          int nparts, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    __shared__ float sh[kBlock / kWave][6];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if ((int)threadIdx.x < nparts) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = partial[threadIdx.x * 6 + a]; hi[a] = partial[threadIdx.x * 6 + 3 + a]; }
    }
    block_bounds(lo, hi, sh);
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    uint32_t key = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float ext = hi[a] - lo[a];
        const float scale = ext > 0.f && ext < INFINITY ? 1024.f / ext : 0.f;      // a zero extent: every point in cell 0
        key |= spread10(knn_cell(pts[(size_t)i * 3 + a], lo[a], scale)) << a;
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

// one wave per box: gather its points into sorted order and fold their bounds
__global__ __launch_bounds__(kBlock) void knn_gather_kernel(int n, int nbox, const float* __restrict__ pts,
                                                            const uint32_t* __restrict__ order, float* __restrict__ sx,
                                                            float* __restrict__ sy, float* __restrict__ sz,
                                                            int32_t* __restrict__ sid, float* __restrict__ box) {
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
    }
}

// (d, j) before (bd, bi) in the order (d2, id)
__device__ __forceinline__ bool knn_before(float d, int j, float bd, int bi) {
    return d < bd || (d == bd && j < bi);
}

// offset o of the outward walk: 0, +1, -1, +2, -2, ...
__device__ __forceinline__ int knn_delta(int o) { return (o & 1) ? (o + 1) >> 1 : -(o >> 1); }

template <int KT>
__global__ __launch_bounds__(kKnnBox) void knn_search_kernel(int n, int nbox, int K, int exclude_self,
                                                             const float* __restrict__ sx, const float* __restrict__ sy,
                                                             const float* __restrict__ sz, const int32_t* __restrict__ sid,
                                                             const float* __restrict__ box, int32_t* __restrict__ idx_out,
                                                             float* __restrict__ d2_out) {
    __shared__ __attribute__((aligned(16))) float cx[kKnnBox], cy[kKnnBox], cz[kKnnBox];
    __shared__ __attribute__((aligned(16))) int cid[kKnnBox];
    const int lane = threadIdx.x, b = blockIdx.x;                  // gridDim.x == nbox
    const size_t p = (size_t)b * kKnnBox + lane;
    const float qx = sx[p], qy = sy[p], qz = sz[p];                // NaN in a padding lane: nothing is ever inserted there
    const int qid = sid[p];
    const bool valid = qid != kNoId;
    const int self = exclude_self ? qid : -1;
    float qlo[3], qhi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { qlo[a] = box[(size_t)a * nbox + b]; qhi[a] = box[(size_t)(3 + a) * nbox + b]; }

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
    const size_t o = (size_t)qid * (size_t)K;                      // qid in [0, n): clamped by the gather
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
int launch_search(int n, int nbox, int K, int exclude_self, const NeighborsTmp& t, int32_t* idx, float* d2, hipStream_t s) {
    OGS_LAUNCH(knn_search_kernel<KT>, dim3((unsigned)nbox), dim3(kKnnBox), 0, s, n, nbox, K, exclude_self, t.sx, t.sy, t.sz,
               t.sid, t.box, idx, d2);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
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
}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_knn_box_points(void) { return kKnnBox; }
size_t ogs_knn_max_k(void) { return kKnnMaxK; }

size_t ogs_knn_neighbors_tmp_bytes(int64_t n) {
    if (n <= 0 || n > (int64_t)INT32_MAX - kKnnBox) return 0;
    return NeighborsTmp::carve(nullptr, n).bytes;
}

int ogs_knn_neighbors(int64_t n, const float* points, int32_t K, int32_t exclude_self, int32_t* idx, float* d2, void* tmp,
                      size_t tmp_bytes, void* stream_) {
    if (n < 0 || n > (int64_t)INT32_MAX - kKnnBox || K < 1 || K > kKnnMaxK || n * (int64_t)K >= ((int64_t)1 << 31)) {
        set_error("knn_neighbors: bad sizes (n=%lld K=%d; 1 <= K <= %d, n * K < 2^31)", (long long)n, K, kKnnMaxK);
        return OGS_ERR_INVALID_ARG;
    }
    if (n == 0) return OGS_OK;
    if (!points || !idx || !d2 || !tmp) { set_error("knn_neighbors: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    const NeighborsTmp t = NeighborsTmp::carve(tmp, n);
    if (tmp_bytes < t.bytes) {
        set_error("knn_neighbors: tmp has %zu bytes, %zu needed (ogs_knn_neighbors_tmp_bytes)", tmp_bytes, t.bytes);
        return OGS_ERR_INVALID_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int ni = (int)n, nbox = (ni + kKnnBox - 1) / kKnnBox;
    const int nparts = min(kBoundBlocks, (ni + kBlock - 1) / kBlock);
    OGS_LAUNCH(knn_bounds_kernel, dim3((unsigned)nparts), dim3(kBlock), 0, s, ni, points, t.partial);
    OGS_LAUNCH_CHECK(0, s);
    OGS_LAUNCH(knn_keys_kernel, dim3((unsigned)((ni + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, ni, points, t.partial, nparts,
               t.keys[0], t.vals[0]);
    OGS_LAUNCH_CHECK(0, s);
    const int shifts[4] = {0, 8, 16, 24}, nbits[4] = {8, 8, 8, 6};  // 30 key bits; an even number of passes ends in [0]
    for (int pass = 0; pass < 4; ++pass) {
        const int in = pass & 1, out = in ^ 1;
        const int rc = radix_pass(t.keys[in], t.vals[in], t.keys[out], t.vals[out], n, shifts[pass], nbits[pass], t.sort_tmp, s, 0);
        if (rc != OGS_OK) return rc;
    }
    const int wpb = kBlock / kWave;
    OGS_LAUNCH(knn_gather_kernel, dim3((unsigned)((nbox + wpb - 1) / wpb)), dim3(kBlock), 0, s, ni, nbox, points, t.vals[0], t.sx,
               t.sy, t.sz, t.sid, t.box);
    OGS_LAUNCH_CHECK(0, s);
    const int ex = exclude_self ? 1 : 0;
    if (K <= 4) return launch_search<4>(ni, nbox, K, ex, t, idx, d2, s);
    if (K <= 8) return launch_search<8>(ni, nbox, K, ex, t, idx, d2, s);
    if (K <= 16) return launch_search<16>(ni, nbox, K, ex, t, idx, d2, s);
    return launch_search<32>(ni, nbox, K, ex, t, idx, d2, s);
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
