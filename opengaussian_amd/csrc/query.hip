// Open-vocabulary queries (include/ogs_query.h): text -> leaves, leaves -> point classes, the confusion table of the
// point-level metrics, and the stable multi-split that lays the rows of overlapping leaf selections out group by group.
//
// None of these kernels waits for another workgroup, every loop bound is an argument, and every index that comes from device
// memory is range-checked before it addresses anything.
//
// This file is compiled with -ffp-contract=off: the similarity is the same chain of fp32 multiplies and adds on every build.
#include "ogs_common.h"
#include "../../include/ogs_query.h"

#include <limits.h>

namespace ogs {
namespace {

constexpr int kQueryWaves = kBlock / kWave;
constexpr int kQueryMaxLeaves = 8192;                   // one query's similarities: 32 KB of LDS
constexpr int kQueryMaxTop = 64;
constexpr int kQueryMaxClasses = 64;                    // 64 * 64 counters: 16 KB of LDS (NYU40 + unlabelled: 41)
constexpr int kConfBlock = 4096;                        // points per workgroup of the confusion table
constexpr int kSplitSteps = 4;                          // 64-row steps of a wave
constexpr int kSplitWaveRows = kSplitSteps * kWave;     // consecutive rows of one wave
constexpr int kSplitBlock = kQueryWaves * kSplitWaveRows;   // rows per workgroup: 1024
constexpr int kSplitMaxGroups = 64;                     // one bit per group in a leaf's uint64
constexpr int kScanItems = 8;                           // consecutive elements per thread and round of the scan
constexpr float kNormEps = 1e-12f;                      // F.normalize

__device__ __forceinline__ float wave_sum(float v) {
    for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// dot(t, l) and |l|^2 over D values, the wave's lanes striding the row: scalar loads up to the first 16-byte boundary of l,
// float4 loads of l over the body (t as float4 too when it is aligned there, else four scalar loads that hit the cache),
// scalar loads for the last D % 4.  The lane partials meet in a butterfly: one fixed order.
__device__ __forceinline__ void row_dot(const float* __restrict__ t, const float* __restrict__ l, int D, int lane, float& dot,
                                        float& sq) {
    const int head = min((int)((0u - (uint32_t)(reinterpret_cast<uintptr_t>(l) >> 2)) & 3u), D);
    const int body = (D - head) >> 2;
    float d = 0.f, s = 0.f;
    if (lane < head) { d = t[lane] * l[lane]; s = l[lane] * l[lane]; }
    const float4* __restrict__ l4 = reinterpret_cast<const float4*>(l + head);
    const float* __restrict__ tb = t + head;
    const bool t_aligned = (reinterpret_cast<uintptr_t>(tb) & 15u) == 0;
    for (int i = lane; i < body; i += kWave) {
        const float4 a = l4[i];
        float4 b;
        if (t_aligned) b = reinterpret_cast<const float4*>(tb)[i];
        else b = make_float4(tb[4 * i], tb[4 * i + 1], tb[4 * i + 2], tb[4 * i + 3]);
        d += (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
        s += (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w);
    }
    const int tail = head + 4 * body + lane;             // fewer than four values are left
    if (tail < D) { d += t[tail] * l[tail]; s += l[tail] * l[tail]; }
    dot = wave_sum(d);
    sq = wave_sum(s);
}

// (value, index) a ranks before (value, index) b: higher value, lower index on ties; index < 0 = nothing
__device__ __forceinline__ bool ranks_before(float av, int ai, float bv, int bi) {
    if (ai < 0) return false;
    if (bi < 0) return true;
    return av > bv || (av == bv && ai < bi);
}

__global__ __launch_bounds__(kBlock) void query_select_kernel(int K, int D, const float* __restrict__ text,
                                                              const float* __restrict__ leaf,
                                                              const uint8_t* __restrict__ leaf_valid,
                                                              const float* __restrict__ centers, int center_dim, float leaf_num,
                                                              float max_dist, int top, float* __restrict__ sim,
                                                              int32_t* __restrict__ selected, int32_t* __restrict__ count) {
    __shared__ float sim_sh[kQueryMaxLeaves];
    __shared__ float wave_v[kQueryWaves];
    __shared__ int wave_i[kQueryWaves];
    __shared__ int rank_sh[kQueryMaxTop];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const float* __restrict__ t = text + (size_t)q * D;

    float tt, tn;
    row_dot(t, t, D, lane, tt, tn);                      // every wave: the same bits
    const float tnorm = fmaxf(sqrtf(tn), kNormEps);
    for (int k = wave; k < K; k += kQueryWaves) {        // one leaf per wave and round
        float v = 0.f;
        if (!leaf_valid || leaf_valid[k]) {              // wave-uniform
            float dot, ln;
            row_dot(t, leaf + (size_t)k * D, D, lane, dot, ln);
            // ONE product and ONE quotient: at D = 1 fl(t * l) / fl(|t| * |l|) is +-1 exactly, as the normalised factors are
            v = dot / (tnorm * fmaxf(sqrtf(ln), kNormEps));
        }
        if (lane == 0) { sim_sh[k] = v; sim[(size_t)q * K + k] = v; }
    }
    if (top <= 0) return;
    __syncthreads();

    // ---- the R highest, one block-wide argmax per rank; a ranked entry becomes NaN in LDS and is never met again ----------
    const int R = min(top, K);
    for (int r = 0; r < R; ++r) {
        float bv = 0.f;
        int bi = -1;
        for (int k = tid; k < K; k += kBlock) {          // ascending k: a later equal value does not replace an earlier one
            const float v = sim_sh[k];
            if (v == v && (bi < 0 || v > bv)) { bv = v; bi = k; }
        }
        for (int m = kWave / 2; m >= 1; m >>= 1) {
            const float ov = __shfl_xor(bv, m, kWave);
            const int oi = __shfl_xor(bi, m, kWave);
            if (ranks_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { wave_v[wave] = bv; wave_i[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kQueryWaves; ++w)
                if (ranks_before(wave_v[w], wave_i[w], bv, bi)) { bv = wave_v[w]; bi = wave_i[w]; }
            rank_sh[r] = bi;                              // -1: nothing but NaN is left
            if (bi >= 0) sim_sh[bi] = __builtin_nanf("");
        }
        __syncthreads();
    }

    // ---- the merge rule of render_lerf_by_text.py:109-115, one thread (at most top - 1 candidates) -------------------------
    if (tid == 0) {
        int32_t* __restrict__ out = selected + (size_t)q * top;
        int n = 0;
        const int best = rank_sh[0];
        if (best >= 0) {
            out[n++] = best;
            for (int r = 1; r < R; ++r) {
                const int c = rank_sh[r];
                if (c < 0) break;
                if (!((float)(c - best) < leaf_num)) continue;
                float d2 = 0.f;
                for (int j = 0; j < center_dim; ++j) {
                    const float d = centers[(size_t)best * center_dim + j] - centers[(size_t)c * center_dim + j];
                    d2 += d * d;
                }
                if (sqrtf(d2) < max_dist) out[n++] = c;
            }
        }
        count[q] = n;
        for (int j = n; j < top; ++j) out[j] = -1;
    }
}

// class_of_leaf[k] = argmax_t sim[t, k], lowest t on ties: one thread per leaf, coalesced over k
__global__ __launch_bounds__(kBlock) void query_leaf_class_kernel(int K, int T, const float* __restrict__ sim,
                                                                  int32_t* __restrict__ class_of_leaf) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= K) return;
    float bv = sim[k];
    int bt = 0;
    for (int t = 1; t < T; ++t) {
        const float v = sim[(size_t)t * K + k];
        if (v > bv) { bv = v; bt = t; }
    }
    class_of_leaf[k] = bt;
}

__global__ __launch_bounds__(kBlock) void query_point_class_kernel(int64_t n, const int64_t* __restrict__ leaf_ind, int K,
                                                                   const int32_t* __restrict__ class_of_leaf,
                                                                   int64_t* __restrict__ pred) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const int64_t id = min(max(leaf_ind[p], (int64_t)0), (int64_t)K - 1);
    pred[p] = (int64_t)class_of_leaf[id] + 1;
}

__global__ __launch_bounds__(kBlock) void query_confusion_kernel(int64_t n, const int64_t* __restrict__ gt,
                                                                 const int64_t* __restrict__ pred,
                                                                 const uint8_t* __restrict__ ignore, int C,
                                                                 unsigned long long* __restrict__ conf) {
    __shared__ uint32_t table[kQueryMaxClasses * kQueryMaxClasses];      // a workgroup meets kConfBlock points: no overflow
    const int cells = C * C;
    for (int c = threadIdx.x; c < cells; c += kBlock) table[c] = 0u;
    __syncthreads();
    const int64_t p0 = (int64_t)blockIdx.x * kConfBlock;
    for (int i = threadIdx.x; i < kConfBlock; i += kBlock) {
        const int64_t p = p0 + i;
        if (p >= n) break;
        const int64_t g = (ignore && ignore[p]) ? 0 : gt[p];
        const int64_t r = g == 0 ? 0 : pred[p];
        if ((uint64_t)g < (uint64_t)C && (uint64_t)r < (uint64_t)C) atomicAdd(&table[(int)g * C + (int)r], 1u);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < cells; c += kBlock) {
        const uint32_t v = table[c];
        if (v) atomicAdd(&conf[c], (unsigned long long)v);
    }
}

// ---- the split ------------------------------------------------------------------------------------------------------------
// tmp: raw [Q * nb] per-(group, workgroup) member counts as the count launch left them, then offs [Q * nb], their exclusive
// prefix over the kept groups; both group-major, so that the prefix runs through group 0's workgroups, then group 1's, ...
struct SplitTmp {
    uint32_t* raw;
    uint32_t* offs;
    static int64_t blocks(int64_t n) { return (n + kSplitBlock - 1) / kSplitBlock; }
    static SplitTmp carve(void* p, int64_t n, int Q) {
        Carver c(p);
        SplitTmp t;
        t.raw = c.take<uint32_t>((size_t)blocks(n) * Q);
        t.offs = c.take<uint32_t>((size_t)blocks(n) * Q);
        return t;
    }
};

__device__ __forceinline__ uint64_t split_membership(int64_t p, int64_t n, const int64_t* __restrict__ leaf_ind, int K,
                                                     const uint64_t* __restrict__ leaf_groups,
                                                     const uint8_t* __restrict__ row_ok, uint64_t group_mask) {
    if (p >= n) return 0ull;
    const int64_t id = leaf_ind[p];
    if (id < 0 || id >= K) return 0ull;                  // the dummy leaf, -1, anything else: no group
    if (row_ok && !row_ok[p]) return 0ull;
    return leaf_groups[id] & group_mask;
}

// The wave's kSplitWaveRows consecutive rows: their membership words into m[], and in lane q the number of members of group q
// among them (one ballot per group and step).
__device__ __forceinline__ uint32_t split_wave_counts(int64_t row0, int64_t n, const int64_t* __restrict__ leaf_ind, int K,
                                                      const uint64_t* __restrict__ leaf_groups,
                                                      const uint8_t* __restrict__ row_ok, int Q, uint64_t group_mask, int lane,
                                                      uint64_t (&m)[kSplitSteps]) {
    uint32_t cnt = 0u;
#pragma unroll
    for (int s = 0; s < kSplitSteps; ++s) {
        m[s] = split_membership(row0 + s * kWave + lane, n, leaf_ind, K, leaf_groups, row_ok, group_mask);
        for (int q = 0; q < Q; ++q) {
            const uint64_t members = __ballot((m[s] >> q) & 1ull);
            if (lane == q) cnt += (uint32_t)__popcll(members);
        }
    }
    return cnt;
}

__device__ __forceinline__ uint64_t low_bits(int Q) { return Q >= 64 ? ~0ull : ((1ull << Q) - 1ull); }

__global__ __launch_bounds__(kBlock) void query_split_count_kernel(int64_t n, const int64_t* __restrict__ leaf_ind, int K,
                                                                   const uint64_t* __restrict__ leaf_groups,
                                                                   const uint8_t* __restrict__ row_ok, int Q, int64_t nb,
                                                                   uint32_t* __restrict__ raw) {
    __shared__ uint32_t wave_cnt[kQueryWaves][kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    uint64_t m[kSplitSteps];
    const int64_t row0 = (int64_t)blockIdx.x * kSplitBlock + wave * kSplitWaveRows;
    wave_cnt[wave][lane] = split_wave_counts(row0, n, leaf_ind, K, leaf_groups, row_ok, Q, low_bits(Q), lane, m);
    __syncthreads();
    if (tid < Q) {
        uint32_t total = 0u;
        for (int w = 0; w < kQueryWaves; ++w) total += wave_cnt[w][tid];
        raw[(size_t)tid * nb + blockIdx.x] = total;
    }
}

// ONE workgroup: exclusive prefix of the E = Q * nb counts (a dropped group counts as empty), kBlock * kScanItems per round
__global__ __launch_bounds__(kBlock) void query_split_scan_kernel(int Q, int64_t nb, const uint8_t* __restrict__ group_keep,
                                                                  const uint32_t* __restrict__ raw, uint32_t* __restrict__ offs,
                                                                  int32_t* __restrict__ begin, int32_t* __restrict__ counts) {
    __shared__ uint32_t wave_total[kQueryWaves];
    __shared__ uint32_t carry_sh;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    if (tid < Q) {                                       // the group totals, before group_keep
        uint32_t total = 0u;
        for (int64_t b = 0; b < nb; ++b) total += raw[(size_t)tid * nb + b];
        counts[tid] = (int32_t)total;
    }
    if (tid == 0) carry_sh = 0u;
    __syncthreads();
    const int64_t E = (int64_t)Q * nb;
    for (int64_t e0 = 0; e0 < E; e0 += (int64_t)kBlock * kScanItems) {
        uint32_t v[kScanItems], mine = 0u;
        const int64_t first = e0 + (int64_t)tid * kScanItems;
#pragma unroll
        for (int i = 0; i < kScanItems; ++i) {
            const int64_t e = first + i;
            v[i] = 0u;
            if (e < E && (!group_keep || group_keep[e / nb])) v[i] = raw[e];
            mine += v[i];
        }
        uint32_t incl = mine;                            // inclusive scan of the thread sums across the wave
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += o;
        }
        if (lane == kWave - 1) wave_total[wave] = incl;
        const uint32_t carry = carry_sh;
        __syncthreads();
        uint32_t run = carry + incl - mine;
        for (int w = 0; w < wave; ++w) run += wave_total[w];
#pragma unroll
        for (int i = 0; i < kScanItems; ++i) {
            const int64_t e = first + i;
            if (e < E) {
                offs[e] = run;
                if (e % nb == 0) begin[e / nb] = (int32_t)run;
            }
            run += v[i];
        }
        __syncthreads();                                 // everyone has read carry_sh and wave_total
        if (tid == kBlock - 1) carry_sh = run;
        __syncthreads();
    }
    if (tid == 0) begin[Q] = (int32_t)carry_sh;
}

__global__ __launch_bounds__(kBlock) void query_split_scatter_kernel(int64_t n, const int64_t* __restrict__ leaf_ind, int K,
                                                                     const uint64_t* __restrict__ leaf_groups,
                                                                     const uint8_t* __restrict__ row_ok, int Q,
                                                                     const uint8_t* __restrict__ group_keep, int64_t nb,
                                                                     const uint32_t* __restrict__ offs, int64_t* __restrict__ rows,
                                                                     int64_t capacity, uint32_t* __restrict__ status_word) {
    __shared__ uint32_t wave_cnt[kQueryWaves][kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint64_t kept = __ballot(lane < Q && (!group_keep || group_keep[lane])) & low_bits(Q);
    uint64_t m[kSplitSteps];
    const int64_t row0 = (int64_t)blockIdx.x * kSplitBlock + wave * kSplitWaveRows;
    wave_cnt[wave][lane] = split_wave_counts(row0, n, leaf_ind, K, leaf_groups, row_ok, Q, kept, lane, m);
    __syncthreads();
    uint32_t base = 0u;                                  // lane q: where this wave's next member of group q goes
    if (lane < Q) {
        base = offs[(size_t)lane * nb + blockIdx.x];
        for (int w = 0; w < wave; ++w) base += wave_cnt[w][lane];
    }
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (kWave - lane));
    bool past = false;
#pragma unroll
    for (int s = 0; s < kSplitSteps; ++s) {
        const int64_t row = row0 + s * kWave + lane;
        for (int q = 0; q < Q; ++q) {
            const bool in = (m[s] >> q) & 1ull;
            const uint64_t members = __ballot(in);
            if (members == 0ull) continue;               // wave-uniform
            const uint32_t at = __shfl(base, q, kWave);
            if (in) {
                const int64_t pos = (int64_t)at + __popcll(members & below);      // ascending rows: ascending positions
                if (pos < capacity) rows[pos] = row; else past = true;
            }
            if (lane == q) base += (uint32_t)__popcll(members);
        }
    }
    if (past) __hip_atomic_fetch_or(status_word, kAsyncSplitOverflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

int split_sizes_ok(const char* what, int64_t n, int32_t Q) {
    if (Q > kSplitMaxGroups) {
        set_error("%s: Q=%d groups, at most %d per call (one bit each in a leaf's word)", what, Q, kSplitMaxGroups);
        return OGS_ERR_UNSUPPORTED;
    }
    if (n < 0 || Q < 0 || (Q > 0 && n > (int64_t)INT32_MAX / Q)) {
        set_error("%s: bad sizes (n=%lld Q=%d; n * Q must fit 31 bits)", what, (long long)n, Q);
        return OGS_ERR_INVALID_ARG;
    }
    return OGS_OK;
}

}  // namespace
}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_query_max_leaves(void) { return kQueryMaxLeaves; }
size_t ogs_query_max_top(void) { return kQueryMaxTop; }
size_t ogs_query_max_classes(void) { return kQueryMaxClasses; }
size_t ogs_query_confusion_block(void) { return kConfBlock; }
size_t ogs_query_split_block(void) { return kSplitBlock; }

size_t ogs_query_split_tmp_bytes(int64_t n, int32_t Q) {
    if (n < 0 || Q < 0) return 0;
    Carver c(nullptr);
    c.take<uint32_t>((size_t)SplitTmp::blocks(n) * Q);
    c.take<uint32_t>((size_t)SplitTmp::blocks(n) * Q);
    return c.off + kAlign;                               // never zero: an empty split still gets a buffer
}

int ogs_query_select(int32_t Q, int32_t K, int32_t D, const float* text, const float* leaf, const uint8_t* leaf_valid,
                     const float* centers, int32_t center_dim, float leaf_num, float max_dist, int32_t top, float* sim,
                     int32_t* selected, int32_t* count, void* stream_) {
    if (Q < 0 || K < 1 || D < 1 || top < 0 || center_dim < 0) {
        set_error("query_select: bad sizes (Q=%d K=%d D=%d top=%d center_dim=%d)", Q, K, D, top, center_dim);
        return OGS_ERR_INVALID_ARG;
    }
    if (K > kQueryMaxLeaves || top > kQueryMaxTop) {
        set_error("query_select: K=%d leaves / top=%d, at most %d / %d (a query's similarities are ranked in LDS)", K, top,
                  kQueryMaxLeaves, kQueryMaxTop);
        return OGS_ERR_UNSUPPORTED;
    }
    if (Q == 0) return OGS_OK;
    if (!text || !leaf || !sim || (top > 0 && (!selected || !count || (center_dim > 0 && !centers)))) {
        set_error("query_select: NULL pointer"); return OGS_ERR_INVALID_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    OGS_LAUNCH(query_select_kernel, dim3((unsigned)Q), dim3(kBlock), 0, s, K, D, text, leaf, leaf_valid, centers, center_dim,
               leaf_num, max_dist, top, sim, selected, count);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

int ogs_query_classify(int64_t n, const int64_t* leaf_ind, int32_t K, int32_t T, const float* sim, int32_t* class_of_leaf,
                       int64_t* pred, void* stream_) {
    if (n < 0 || K < 1 || T < 1) {
        set_error("query_classify: bad sizes (n=%lld K=%d T=%d)", (long long)n, K, T); return OGS_ERR_INVALID_ARG;
    }
    if (!sim || !class_of_leaf || (n > 0 && (!leaf_ind || !pred))) {
        set_error("query_classify: NULL pointer"); return OGS_ERR_INVALID_ARG;
    }
    if ((n + kBlock - 1) / kBlock > (int64_t)INT32_MAX) {
        set_error("query_classify: n=%lld is more than one launch covers", (long long)n); return OGS_ERR_UNSUPPORTED;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    OGS_LAUNCH(query_leaf_class_kernel, dim3((unsigned)((K + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, K, T, sim,
               class_of_leaf);
    OGS_LAUNCH_CHECK(0, s);
    if (n == 0) return OGS_OK;
    OGS_LAUNCH(query_point_class_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, n, leaf_ind, K,
               class_of_leaf, pred);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

int ogs_query_confusion(int64_t n, const int64_t* gt, const int64_t* pred, const uint8_t* ignore, int32_t C, int64_t* conf,
                        void* stream_) {
    if (n < 0 || C < 1) { set_error("query_confusion: bad sizes (n=%lld C=%d)", (long long)n, C); return OGS_ERR_INVALID_ARG; }
    if (C > kQueryMaxClasses) {
        set_error("query_confusion: %d classes, at most %d (the table of a workgroup lives in LDS)", C, kQueryMaxClasses);
        return OGS_ERR_UNSUPPORTED;
    }
    if (!conf || (n > 0 && (!gt || !pred))) { set_error("query_confusion: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    if ((n + kConfBlock - 1) / kConfBlock > (int64_t)INT32_MAX) {
        set_error("query_confusion: n=%lld is more than one launch covers", (long long)n); return OGS_ERR_UNSUPPORTED;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    OGS_HIP_CHECK(hipMemsetAsync(conf, 0, sizeof(int64_t) * (size_t)C * C, s));
    if (n == 0) return OGS_OK;
    OGS_LAUNCH(query_confusion_kernel, dim3((unsigned)((n + kConfBlock - 1) / kConfBlock)), dim3(kBlock), 0, s, n, gt, pred,
               ignore, C, reinterpret_cast<unsigned long long*>(conf));
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

int ogs_query_split_count(int64_t n, const int64_t* leaf_ind, int32_t K, const uint64_t* leaf_groups, const uint8_t* row_ok,
                          int32_t Q, void* tmp, void* stream_) {
    const int rc = split_sizes_ok("query_split_count", n, Q);
    if (rc != OGS_OK) return rc;
    if (K < 0) { set_error("query_split_count: K=%d", K); return OGS_ERR_INVALID_ARG; }
    if (n == 0 || Q == 0) return OGS_OK;
    if (!leaf_ind || !leaf_groups || !tmp) { set_error("query_split_count: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const SplitTmp t = SplitTmp::carve(tmp, n, Q);
    const int64_t nb = SplitTmp::blocks(n);
    OGS_LAUNCH(query_split_count_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, n, leaf_ind, K, leaf_groups, row_ok, Q, nb,
               t.raw);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

int ogs_query_split_scan(int64_t n, int32_t Q, const uint8_t* group_keep, void* tmp, int32_t* begin, int32_t* counts,
                         void* stream_) {
    const int rc = split_sizes_ok("query_split_scan", n, Q);
    if (rc != OGS_OK) return rc;
    if (!begin || (Q > 0 && !counts)) { set_error("query_split_scan: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (n == 0 || Q == 0) {                              // no rows: every group is empty
        OGS_HIP_CHECK(hipMemsetAsync(begin, 0, sizeof(int32_t) * ((size_t)Q + 1), s));
        if (Q > 0) OGS_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)Q, s));
        return OGS_OK;
    }
    if (!tmp) { set_error("query_split_scan: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    const SplitTmp t = SplitTmp::carve(tmp, n, Q);
    OGS_LAUNCH(query_split_scan_kernel, dim3(1), dim3(kBlock), 0, s, Q, SplitTmp::blocks(n), group_keep, t.raw, t.offs, begin,
               counts);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

int ogs_query_split_scatter(int64_t n, const int64_t* leaf_ind, int32_t K, const uint64_t* leaf_groups,
                            const uint8_t* row_ok, int32_t Q, const uint8_t* group_keep, const void* tmp, int64_t* rows,
                            int64_t capacity, void* stream_) {
    const int rc = split_sizes_ok("query_split_scatter", n, Q);
    if (rc != OGS_OK) return rc;
    if (K < 0 || capacity < 0) {
        set_error("query_split_scatter: K=%d capacity=%lld", K, (long long)capacity); return OGS_ERR_INVALID_ARG;
    }
    if (n == 0 || Q == 0 || capacity == 0) return OGS_OK;
    if (!leaf_ind || !leaf_groups || !tmp || !rows) { set_error("query_split_scatter: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    uint32_t* status_word = async_status_word();
    if (!status_word) return OGS_ERR_HIP;
    const SplitTmp t = SplitTmp::carve(const_cast<void*>(tmp), n, Q);
    const int64_t nb = SplitTmp::blocks(n);
    OGS_LAUNCH(query_split_scatter_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, n, leaf_ind, K, leaf_groups, row_ok, Q,
               group_keep, nb, t.offs, rows, capacity, status_word);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

}  // extern "C"
