// Exact k-nearest-distance sums per group (include/ogs_knn.h): for every row the K smallest squared distances to the rows
// of its own group, as (K-th value, fp64 sum, fp64 sum of squares).  Brute force, no n x n buffer, no neighbour list.
//
// K reaches several hundred (K = sqrt(n)), so a per-thread top-K list does not fit in registers.  The K-th smallest value
// is found by THRESHOLD SELECTION instead: the bit pattern of a non-negative float is monotone in its value, so the K-th
// smallest d2 is the smallest pattern t with count(d2 <= t) >= K -- a bisection over [0, +inf] = [0, 0x7f800000], 31
// counting passes over the group whatever K is.  One more pass sums what lies below the threshold in fp64; ties at the
// threshold enter K - count_below times, so the sums are those of a sort.
//
// Mapping: a workgroup owns 64 * Q consecutive rows (its QUERIES: lane l of every wave holds rows l, l + 64, ...) and walks
// the point range of the groups those rows belong to in tiles of kKnnTile points staged in LDS, coordinate by coordinate.  The
// four waves split every tile into four slices: all lanes of a wave read the same four points (broadcast ds_read_b128), each
// against its own queries, and the four partial counts of a query meet in LDS once per pass.  Splitting the points, not only
// the queries, across waves is what fills the chip at a few ten thousand rows.  A range that fits one tile (the leaf-sized
// groups of render()) is staged once for all 32 passes.
//
// This file is compiled with -ffp-contract=off: d2 = (dx*dx + dy*dy) + dz*dz, exactly so.
#include "ogs_common.h"
#include "../../include/ogs_knn.h"

#include <limits.h>

// queries per thread (1 or 2), 0 = by size (ogs_knn_group_ksum); a build switch for A-B timing only
#ifndef OGS_KNN_FORCE_Q
#define OGS_KNN_FORCE_Q 0
#endif

namespace ogs {
namespace {

constexpr int kKnnWaves = kBlock / kWave;               // slices of a tile
constexpr int kKnnTile = 1024;                          // points per tile: 12 KB of LDS
constexpr int kKnnSlice = kKnnTile / kKnnWaves;
constexpr int kKnnLoads = kKnnTile / kBlock;            // points a thread stages per tile
constexpr int kKnnStep = 8;                             // points per step of the inner loop (two 4-point reads)
constexpr uint32_t kInfBits = 0x7f800000u;
constexpr int kKnnPasses = 31;                          // ceil(log2(kInfBits + 1))
constexpr int kKnnTwoQueriesFrom = 16384;                // rows from which a thread takes two queries (ogs_knn_group_ksum)
constexpr uint32_t kNever = 0xFFFFFFFFu;                // above every threshold: a point outside the query's group
static_assert(kKnnSlice % kKnnStep == 0 && kKnnStep % 4 == 0, "a slice is a whole number of steps of 4-point reads");

__device__ __forceinline__ int wave_min_int(int v) {
    for (int m = kWave / 2; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, kWave));
    return v;
}
__device__ __forceinline__ int wave_max_int(int v) {
    for (int m = kWave / 2; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, kWave));
    return v;
}

// One wave's slice of a tile against the wave's queries.  The tile is stored coordinate by coordinate (x[], y[], z[]), so
// that one ds_read_b128 per coordinate brings FOUR points: 3 LDS cycles per point, where a 16-byte point record costs 4 and
// a 12-byte one 8.  The slice is padded with NaN points past the end of the range (their d2 is a NaN: above every
// threshold as a bit pattern), so `npts` is rounded up to the step by the caller.
// MASKED: the queries of the workgroup sit in different groups, a point counts only inside the query's own [beg, beg + len).
// SUM: the last pass -- count and sum what lies strictly below the threshold.
template <int Q, bool MASKED, bool SUM>
__device__ __forceinline__ void knn_slice(const float* __restrict__ sx, const float* __restrict__ sy,
                                          const float* __restrict__ sz, int npts, int jbase, const float (&px)[Q],
                                          const float (&py)[Q], const float (&pz)[Q], const int (&beg)[Q],
                                          const int (&len)[Q], const uint32_t (&thr)[Q], int (&cnt)[Q], double (&s1)[Q],
                                          double (&s2)[Q]) {
#pragma unroll 1
    for (int p0 = 0; p0 < npts; p0 += kKnnStep) {                   // (left to itself hipcc unrolls this into 256 VGPRs)
#pragma unroll
        for (int v = 0; v < kKnnStep; v += 4) {
            const float4 x4 = *reinterpret_cast<const float4*>(sx + p0 + v);
            const float4 y4 = *reinterpret_cast<const float4*>(sy + p0 + v);
            const float4 z4 = *reinterpret_cast<const float4*>(sz + p0 + v);
            const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, ys[4] = {y4.x, y4.y, y4.z, y4.w}, zs[4] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const float dx = px[q] - xs[u], dy = py[q] - ys[u], dz = pz[q] - zs[u];
                    const float d = (dx * dx + dy * dy) + dz * dz;
                    uint32_t bits = __float_as_uint(d);
                    if (MASKED) bits = (uint32_t)(jbase + p0 + v + u - beg[q]) < (uint32_t)len[q] ? bits : kNever;
                    if (!SUM) {
                        cnt[q] += bits <= thr[q] ? 1 : 0;
                    } else {
                        const bool below = bits < thr[q];
                        const double dd = below ? (double)d : 0.0;
                        cnt[q] += below ? 1 : 0;
                        s1[q] += dd;
                        s2[q] += dd * dd;
                    }
                }
            }
        }
    }
}

template <int Q>
__global__ __launch_bounds__(kBlock) void knn_group_ksum_kernel(int n, const float* __restrict__ pts, int G,
                                                                const int32_t* __restrict__ group_begin,
                                                                const int32_t* __restrict__ group_k,
                                                                float* __restrict__ kth_out, double* __restrict__ sum1,
                                                                double* __restrict__ sum2) {
    constexpr int QB = kWave * Q;                       // queries of the workgroup
    __shared__ __attribute__((aligned(16))) float tile_x[kKnnTile], tile_y[kKnnTile], tile_z[kKnnTile];
    __shared__ int cnt_sh[2][kKnnWaves][QB];            // by pass parity: one barrier per pass
    __shared__ double acc_sh[kKnnWaves][QB][2];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;

    // ---- the queries: every wave holds the same QB rows --------------------------------------------------------------
    int row[Q], beg[Q], len[Q], K[Q];
    bool valid[Q];
    float px[Q], py[Q], pz[Q];
    int minb = INT_MAX, maxb = -1, mine = INT_MAX, maxe = -1;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int64_t r = (int64_t)blockIdx.x * QB + q * kWave + lane;
        row[q] = r < n ? (int)r : -1;
        beg[q] = len[q] = K[q] = 0;
        px[q] = py[q] = pz[q] = 0.f;
        valid[q] = false;
        if (row[q] >= 0) {
            int a = 0, b = G + 1;                        // first index with group_begin[index] > row
            while (a < b) {
                const int m = (a + b) >> 1;
                if (group_begin[m] <= row[q]) a = m + 1; else b = m;
            }
            const int g = a - 1;                         // -1: before the first group; G: after the last
            if (g >= 0 && g < G) {
                const int b0 = min(max(group_begin[g], 0), n), e0 = min(max(group_begin[g + 1], b0), n);
                if (row[q] >= b0 && row[q] < e0) {       // always, for non-decreasing offsets
                    valid[q] = true;
                    beg[q] = b0;
                    len[q] = e0 - b0;
                    K[q] = min(max(group_k[g], 0), len[q]);
                    px[q] = pts[(size_t)row[q] * 3]; py[q] = pts[(size_t)row[q] * 3 + 1]; pz[q] = pts[(size_t)row[q] * 3 + 2];
                    minb = min(minb, b0); maxb = max(maxb, b0);
                    mine = min(mine, e0); maxe = max(maxe, e0);
                }
            }
        }
    }
    minb = wave_min_int(minb); maxb = wave_max_int(maxb);
    mine = wave_min_int(mine); maxe = wave_max_int(maxe);
    if (maxe < 0) return;                                // no row of this workgroup is in a group (all waves agree)
    const int lo = minb, hi = maxe;                      // the point range the workgroup walks; 0 <= lo < hi <= n
    const bool one_group = minb == maxb && mine == maxe;
    const int ntiles = (hi - lo + kKnnTile - 1) / kKnnTile;
    const bool single = ntiles == 1;

    // ---- staging: registers -> LDS, the next tile's loads in flight while this one is consumed -------------------------
    float stage[kKnnLoads][3];
    auto fetch = [&](int t) {
#pragma unroll
        for (int k = 0; k < kKnnLoads; ++k) {
            const int j = lo + t * kKnnTile + k * kBlock + tid;
            const bool in = j < hi;
            const size_t o = (size_t)(in ? j : lo) * 3;
            const float x = pts[o], y = pts[o + 1], z = pts[o + 2];
            stage[k][0] = in ? x : __builtin_nanf("");
            stage[k][1] = in ? y : __builtin_nanf("");
            stage[k][2] = in ? z : __builtin_nanf("");
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int k = 0; k < kKnnLoads; ++k) {
            tile_x[k * kBlock + tid] = stage[k][0]; tile_y[k * kBlock + tid] = stage[k][1]; tile_z[k * kBlock + tid] = stage[k][2];
        }
    };
    fetch(0);
    if (single) { stash(); __syncthreads(); }

    uint32_t blo[Q], bhi[Q];                              // the K-th value's bit pattern lies in [blo, bhi]
#pragma unroll
    for (int q = 0; q < Q; ++q) { blo[q] = 0u; bhi[q] = kInfBits; }

    for (int pass = 0; pass <= kKnnPasses; ++pass) {
        const bool last = pass == kKnnPasses;
        uint32_t thr[Q];
        int cnt[Q];
        double s1[Q], s2[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            thr[q] = last ? bhi[q] : blo[q] + ((bhi[q] - blo[q]) >> 1);
            cnt[q] = 0; s1[q] = 0.0; s2[q] = 0.0;
        }
        for (int t = 0; t < ntiles; ++t) {
            if (!single) {
                __syncthreads();                          // every wave is done with the tile in LDS
                stash();
                __syncthreads();
                fetch(t + 1 < ntiles ? t + 1 : 0);        // (after the very last tile: one unused in-range load)
            }
            const int jbase = lo + t * kKnnTile + wave * kKnnSlice;
            int npts = min(kKnnSlice, hi - jbase);
            if (npts <= 0) continue;                      // wave-uniform
            npts = (npts + kKnnStep - 1) / kKnnStep * kKnnStep;
            const float *sx = tile_x + wave * kKnnSlice, *sy = tile_y + wave * kKnnSlice, *sz = tile_z + wave * kKnnSlice;
            if (one_group) {
                if (!last) knn_slice<Q, false, false>(sx, sy, sz, npts, jbase, px, py, pz, beg, len, thr, cnt, s1, s2);
                else knn_slice<Q, false, true>(sx, sy, sz, npts, jbase, px, py, pz, beg, len, thr, cnt, s1, s2);
            } else {
                if (!last) knn_slice<Q, true, false>(sx, sy, sz, npts, jbase, px, py, pz, beg, len, thr, cnt, s1, s2);
                else knn_slice<Q, true, true>(sx, sy, sz, npts, jbase, px, py, pz, beg, len, thr, cnt, s1, s2);
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            cnt_sh[pass & 1][wave][q * kWave + lane] = cnt[q];
            if (last) { acc_sh[wave][q * kWave + lane][0] = s1[q]; acc_sh[wave][q * kWave + lane][1] = s2[q]; }
        }
        __syncthreads();
        if (!last) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                int total = 0;
#pragma unroll
                for (int w = 0; w < kKnnWaves; ++w) total += cnt_sh[pass & 1][w][q * kWave + lane];
                // count(d2 <= bhi) >= K holds throughout (K <= len, all d2 finite); once blo == bhi nothing moves
                if (total >= K[q]) bhi[q] = thr[q]; else blo[q] = thr[q] + 1u;
            }
        } else if (wave == 0) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                if (!valid[q]) continue;
                int below = 0;
                double a1 = 0.0, a2 = 0.0;
#pragma unroll
                for (int w = 0; w < kKnnWaves; ++w) {      // slices in point order: a fixed summation order
                    below += cnt_sh[pass & 1][w][q * kWave + lane];
                    a1 += acc_sh[w][q * kWave + lane][0];
                    a2 += acc_sh[w][q * kWave + lane][1];
                }
                float kv = 0.f;
                if (K[q] > 0) {
                    kv = __uint_as_float(bhi[q]);
                    const double ties = (double)(K[q] - below), kd = (double)kv;
                    a1 += ties * kd;
                    a2 += ties * (kd * kd);
                } else {
                    a1 = a2 = 0.0;
                }
                if (kth_out) kth_out[row[q]] = kv;
                sum1[row[q]] = a1;
                sum2[row[q]] = a2;
            }
        }
    }
}

template <int Q>
int launch_knn(int n, const float* pts, int G, const int32_t* gb, const int32_t* gk, float* kth, double* sum1, double* sum2,
               hipStream_t s) {
    const int qb = kWave * Q;
    OGS_LAUNCH(knn_group_ksum_kernel<Q>, dim3((unsigned)(((int64_t)n + qb - 1) / qb)), dim3(kBlock), 0, s, n, pts, G, gb, gk,
               kth, sum1, sum2);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

}  // namespace
}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_knn_tile_points(void) { return kKnnTile; }

int ogs_knn_group_ksum(int64_t n, const float* points, int32_t G, const int32_t* group_begin, const int32_t* group_k,
                       float* kth, double* sum1, double* sum2, void* stream_) {
    if (n < 0 || n > (int64_t)INT32_MAX - kKnnTile || G < 0) {          // point indices of a padded tile stay in int32
        set_error("knn_group_ksum: bad sizes (n=%lld G=%d)", (long long)n, G);
        return OGS_ERR_INVALID_ARG;
    }
    if (n == 0 || G == 0) return OGS_OK;
    if (!points || !group_begin || !group_k || !sum1 || !sum2) {
        set_error("knn_group_ksum: NULL pointer"); return OGS_ERR_INVALID_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    // Two queries per thread halve the LDS reads per distance (one broadcast read feeds both) and the number of workgroups.
    // Measured (scripts/knn_filter_bench.py --only-new, one group): 5 000 rows 1.28 ms at Q = 1 against 1.61 at Q = 2;
    // 20 000 rows 6.47 against 5.89; 50 000 rows 28.7 against 23.7; 100 000 rows 91.2 against 90.1; Q = 4 (one wave per SIMD
    // by registers) lost at every size.  The switch sits between the first two sizes; the result does not depend on Q.
    int q = n >= kKnnTwoQueriesFrom ? 2 : 1;
    if (OGS_KNN_FORCE_Q) q = OGS_KNN_FORCE_Q;
    if (q == 2) return launch_knn<2>((int)n, points, G, group_begin, group_k, kth, sum1, sum2, s);
    return launch_knn<1>((int)n, points, G, group_begin, group_k, kth, sum1, sum2, s);
}

}  // extern "C"
