// Wide k-means on gfx950: codebooks for per-Gaussian feature vectors up to 1024-D (C ABI: include/ogs_kmeans.h,
// the ogs_kmeans_wide_* block).  csrc/kmeans.hip stays the codebook of the reference's 6 / 9-D instance features.
//
// Scoring pass.  argmin_c |x - c|^2 = argmax_c (x.c - |c|^2 / 2) and the cosine arg-max is argmax_c x.c on unit centres:
// one N x D x k contraction plus a bias per centre, and it runs on the matrix pipe.  fp32 accuracy comes from the
// truncation split of kmeans_gemm_pass_kernel: every operand is hi + mid + lo, three bf16 terms that carry its 24
// significant bits exactly, and of the nine cross products the six with weight >= 2^-16 are kept (hh, hm, hl, mh, mm, lh;
// the dropped ones are <= 2^-22 relative each).  Every bf16 x bf16 product is exact in fp32, the sum is the MFMA's fp32
// accumulator, smallest terms first.  Six v_mfma_f32_16x16x32_bf16 (16 cycles each) cover 16 x 16 x 32 products; the exact
// fp32 form v_mfma_f32_16x16x4_f32 needs eight instructions of 32 cycles for them.
//   * Centres are split and packed ONCE per pass (wide_pack_kernel) in the order the MFMA wants its A operand: one 16-byte
//     load per lane, plane and K step, no vector work on the centre side of the inner loop.  The bias lies beside them in
//     fp32 (-|c'|^2 / 2, 0 for cosine, -inf for the padding centres of the last tile, which therefore never win).
//   * A workgroup owns a row tile.  Its rows are split once, into LDS, in B-operand order (one ds_read_b128 per lane, plane
//     and K step, conflict free); its 4, 8 or 16 waves take the centre tiles round robin and all of them read the same rows.
//     The tile is 64 rows while the three planes fit (6 B per element: D <= 384), 48 up to D = 512, 32 up to 768, 16 beyond.
//   * L2: both sides are shifted by the centroid of a fixed sample of the rows (wide_shift_kernel; a function of the data
//     alone), so the magnitudes that cancel in x.c - |c|^2 / 2 are the spread of the data, not its distance from the origin.
//   * The running (best score, best id) stays in registers: per lane a strict compare in centre order, then the partial
//     winners of a row (every wave's 4 lane groups) are merged on (score, lower index).  No [N, k] buffer exists.
//   * More than kStage centres are packed and scored in stages of kStage; the best score of a row crosses stages in tmp.
// `dist` is recomputed for the winner from the fp32 inputs (differences first), never derived from the score.
//
// Centre update: no float atomics.  ogs_knn_transpose (K = 1, R = k) turns the ids into each centre's ascending row list,
// ogs_knn_aggregate_t sums w x over it in the fixed order include/ogs_knn.h states (and, with a column of ones, w itself);
// wide_finalize_kernel divides, normalises for cosine and keeps an empty centre's bytes.
#include "ogs_common.h"
#include "../../include/ogs_kmeans.h"
#include "../../include/ogs_knn.h"

#include <limits>

namespace ogs {

namespace {

constexpr int kDimStep = 32;         // K of one MFMA: D is padded to a multiple of it
constexpr int kCentreTile = 16;      // centres of one accumulator tile
constexpr int kRowTile = 64;         // rows of a workgroup while the planes fit (wide_row_tiles)
constexpr int kWideMaxDim = 1024;
constexpr int kWideMaxK = 16384;
constexpr int kStage = 4096;         // centres packed at a time: at most 24 MiB of planes at D = 1024
constexpr int kWideShiftRows = 64;   // rows behind the L2 shift
constexpr int kInertiaBlocks = 256;
constexpr int kWideMaxBlock = 1024;  // threads of a scoring workgroup: 256, 512 or 1024 (wide_threads)
constexpr size_t kPlanesLds = 144 * 1024;   // what the row planes may take of the 160 KiB

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned pack_hi16(float lo_elem, float hi_elem) {      // {bf16(lo_elem), bf16(hi_elem)} by truncation
    return __builtin_amdgcn_perm(__float_as_uint(hi_elem), __float_as_uint(lo_elem), 0x07060302u);
}
// v[0..8) -> the three bf16 planes of the truncation split: h = top 16 bits, m = top 16 bits of v - h, l = v - h - m (exact,
// at most 8 significant bits)
__device__ __forceinline__ void split_planes(const float (&v)[8], u32x4& ph, u32x4& pm, u32x4& pl) {
    float h[8], m[8], l[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        h[i] = __uint_as_float(__float_as_uint(v[i]) & 0xFFFF0000u);
        const float r = v[i] - h[i];
        m[i] = __uint_as_float(__float_as_uint(r) & 0xFFFF0000u);
        l[i] = r - m[i];
    }
    ph = u32x4{pack_hi16(h[0], h[1]), pack_hi16(h[2], h[3]), pack_hi16(h[4], h[5]), pack_hi16(h[6], h[7])};
    pm = u32x4{pack_hi16(m[0], m[1]), pack_hi16(m[2], m[3]), pack_hi16(m[4], m[5]), pack_hi16(m[6], m[7])};
    pl = u32x4{pack_hi16(l[0], l[1]), pack_hi16(l[2], l[3]), pack_hi16(l[4], l[5]), pack_hi16(l[6], l[7])};
}

// src[0..D) of one row, dimensions d0 .. d0 + 7 minus the shift, zero past D (or when the row does not exist)
__device__ __forceinline__ void load8_shifted(const float* __restrict__ src, bool exists, int d0, int D, bool vec,
                                              const float* __restrict__ mu, float (&v)[8]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int d = d0 + 4 * h;
        if (exists && vec && d + 4 <= D) {
            const float4 q = *reinterpret_cast<const float4*>(src + d);
            v[4 * h + 0] = q.x - mu[d];
            v[4 * h + 1] = q.y - mu[d + 1];
            v[4 * h + 2] = q.z - mu[d + 2];
            v[4 * h + 3] = q.w - mu[d + 3];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[4 * h + i] = (exists && d + i < D) ? src[d + i] - mu[d + i] : 0.f;
        }
    }
}

// mu[0..Dpad): L2 -- the centroid of the rows 0, step, 2 step, ... (ns = min(N, kWideShiftRows), step = N / ns), summed in
// row order; cosine and the padding -- zero.  One workgroup.
__global__ __launch_bounds__(kBlock) void wide_shift_kernel(const float* __restrict__ X, int64_t N, int D, int Dpad, int metric,
                                                            float* __restrict__ mu) {
    const int ns = (int)min(N, (int64_t)kWideShiftRows);
    const int64_t step = ns > 0 ? N / ns : 0;
    for (int c = threadIdx.x; c < Dpad; c += kBlock) {
        float m = 0.f;
        if (metric == OGS_KMEANS_WIDE_L2 && c < D && ns > 0) {
            for (int i = 0; i < ns; ++i) m += X[i * step * D + c];
            m = m / (float)ns;
        }
        mu[c] = m;
    }
}

// One centre tile per workgroup: planes[((ct * KC + kc) * 3 + plane) * 64 + lane], lane (j = lane & 15, g = lane >> 4) holding
// centre c0 + 16 ct + j, dimensions 32 kc + 8 g .. + 7 -- the A operand of v_mfma_f32_16x16x32_bf16 as it is loaded.
__global__ __launch_bounds__(kBlock) void wide_pack_kernel(const float* __restrict__ C, int k, int D, int KC, int c0, int metric,
                                                           const float* __restrict__ mu, u32x4* __restrict__ planes,
                                                           float* __restrict__ bias) {
    const int ct = blockIdx.x, tid = threadIdx.x;
    const bool vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(C) & 15u) == 0;
    for (int e = tid; e < KC * 64; e += kBlock) {
        const int kc = e >> 6, lane = e & 63, j = lane & 15, g = lane >> 4;
        const int c = c0 + ct * kCentreTile + j;
        float v[8];
        load8_shifted(C + (int64_t)min(c, k - 1) * D, c < k, kc * kDimStep + 8 * g, D, vec, mu, v);
        u32x4 ph, pm, pl;
        split_planes(v, ph, pm, pl);
        u32x4* dst = planes + ((size_t)(ct * KC + kc) * 3) * 64 + lane;
        dst[0] = ph;
        dst[64] = pm;
        dst[128] = pl;
    }
    // bias: 16 lanes per centre, each a chain over its columns, folded pairwise -- one fixed order
    const int j = tid >> 4, l = tid & 15;
    const int c = c0 + ct * kCentreTile + j;
    float n2 = 0.f;
    if (c < k && metric == OGS_KMEANS_WIDE_L2)
        for (int d = l; d < D; d += 16) {
            const float t = C[(int64_t)c * D + d] - mu[d];
            n2 = fmaf(t, t, n2);
        }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) n2 += __shfl_xor(n2, m, 16);
    if (l == 0) bias[ct * kCentreTile + j] = c < k ? -0.5f * n2 : -std::numeric_limits<float>::infinity();
}

// Scores of one row tile against one stage of packed centres, arg-max, and (last stage) the winner's distance.
// NT: 16-row sub-tiles per workgroup.  LDS: 3 * NT * KC * 64 u32x4 of row planes; the merge table reuses it after the scoring.
template <int NT>
__global__ __launch_bounds__(kWideMaxBlock) void wide_score_kernel(const float* __restrict__ X, int64_t N, int D, int KC,
                                                            const u32x4* __restrict__ planes, const float* __restrict__ bias,
                                                            int nct, int c0, int first, int last, int metric,
                                                            const float* __restrict__ mu, const float* __restrict__ C,
                                                            float* __restrict__ best_io, int32_t* __restrict__ ids,
                                                            float* __restrict__ dist) {
    constexpr int RT = NT * 16;
    extern __shared__ u32x4 smem[];
    u32x4* rows = smem;                                                   // [3][NT][KC][64]
    const int nthreads = blockDim.x, nwaves = nthreads / kWave;
    const int slots = 4 * nwaves;                                    // partial winners of a row: one per wave and lane group
    float* ms = reinterpret_cast<float*>(smem);                           // [RT][slots] partial winners: score   (after the scoring)
    int* mi = reinterpret_cast<int*>(ms + RT * slots);                   // [RT][slots]                   id
    int* fin = mi + RT * slots;                                          // [RT] merged ids
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * RT;
    const bool vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15u) == 0;

    // ---- the tile's rows: shifted, split, laid out as B operands.  Consecutive threads take consecutive rows of one 8-column
    // group: a wave reads 16 whole 128-byte lines and writes 64 consecutive 16-byte slots per plane
    const int G8 = KC * 4;
    for (int e = tid; e < RT * G8; e += nthreads) {
        const int jj = e & 15, q = e >> 4, grp = q % G8, nt = q / G8;
        const int64_t row = row0 + nt * 16 + jj;
        float v[8];
        load8_shifted(X + min(row, N - 1) * D, row < N, grp * 8, D, vec, mu, v);
        u32x4 ph, pm, pl;
        split_planes(v, ph, pm, pl);
        const int slot = (grp & 3) * 16 + jj, kc = grp >> 2;
        rows[((size_t)(0 * NT + nt) * KC + kc) * 64 + slot] = ph;
        rows[((size_t)(1 * NT + nt) * KC + kc) * 64 + slot] = pm;
        rows[((size_t)(2 * NT + nt) * KC + kc) * 64 + slot] = pl;
    }
    __syncthreads();

    // ---- scores: lane (j, g) ends up with centre 16 ct + 4 g + r, row 16 nt + j in acc[nt][r]
    const float ninf = -std::numeric_limits<float>::infinity();
    float best[NT];
    int bid[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { best[nt] = ninf; bid[nt] = c0; }
    for (int ct = wave; ct < nct; ct += nwaves) {
        floatx4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = floatx4{0.f, 0.f, 0.f, 0.f};
        const u32x4* ap = planes + (size_t)ct * KC * 192 + lane;
        u32x4 ah = ap[0], am = ap[64], al = ap[128];
        for (int kc = 0; kc < KC; ++kc) {
            const u32x4 ch = ah, cm = am, cl = al;
            if (kc + 1 < KC) {                                            // the next step's centre planes, one step ahead
                ah = ap[(kc + 1) * 192];
                am = ap[(kc + 1) * 192 + 64];
                al = ap[(kc + 1) * 192 + 128];
            }
            const bf16x8_t Ah = __builtin_bit_cast(bf16x8_t, ch), Am = __builtin_bit_cast(bf16x8_t, cm),
                           Al = __builtin_bit_cast(bf16x8_t, cl);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const bf16x8_t Bh = __builtin_bit_cast(bf16x8_t, rows[((size_t)(0 * NT + nt) * KC + kc) * 64 + lane]);
                const bf16x8_t Bm = __builtin_bit_cast(bf16x8_t, rows[((size_t)(1 * NT + nt) * KC + kc) * 64 + lane]);
                const bf16x8_t Bl = __builtin_bit_cast(bf16x8_t, rows[((size_t)(2 * NT + nt) * KC + kc) * 64 + lane]);
                floatx4 a = acc[nt];
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al, Bh, a, 0, 0, 0);      // smallest terms first
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bl, a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Am, Bm, a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Am, Bh, a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bm, a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bh, a, 0, 0, 0);
                acc[nt] = a;
            }
        }
        const float4 b4 = *reinterpret_cast<const float4*>(bias + ct * kCentreTile + 4 * g);
        const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
        const int cbase = c0 + ct * kCentreTile + 4 * g;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float sc = acc[nt][r] + bb[r];
                if (sc > best[nt]) { best[nt] = sc; bid[nt] = cbase + r; }           // strict: the lower index keeps a tie
            }
    }
    __syncthreads();                                                      // every wave is done with the row planes
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        ms[(nt * 16 + j) * slots + wave * 4 + g] = best[nt];
        mi[(nt * 16 + j) * slots + wave * 4 + g] = bid[nt];
    }
    __syncthreads();
    if (tid < RT) {
        const int64_t row = row0 + tid;
        const bool live = row < N;
        float bs = ninf;
        int bi = c0;
        if (!first && live) { bs = best_io[row]; bi = ids[row]; }
        for (int s = 0; s < slots; ++s) {
            const float sc = ms[tid * slots + s];
            const int id = mi[tid * slots + s];
            if (sc > bs || (sc == bs && id < bi)) { bs = sc; bi = id; }
        }
        fin[tid] = bi;
        if (live) {
            ids[row] = bi;
            if (!last) best_io[row] = bs;
        }
    }
    if (!last || !dist) return;
    __syncthreads();
    // ---- the winner's distance from the fp32 inputs: one wave per row, every lane a chain over its columns, folded pairwise
    for (int r = wave; r < RT; r += nwaves) {
        const int64_t row = row0 + r;
        if (row >= N) break;
        const float* x = X + row * D;
        const float* c = C + (int64_t)fin[r] * D;
        float a0 = 0.f, a1 = 0.f;
        if (metric == OGS_KMEANS_WIDE_L2) {
            for (int d = lane; d < D; d += kWave) {
                const float t = x[d] - c[d];
                a0 = fmaf(t, t, a0);
            }
        } else {
            for (int d = lane; d < D; d += kWave) {
                a0 = fmaf(x[d], c[d], a0);
                a1 = fmaf(x[d], x[d], a1);
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            a0 += __shfl_xor(a0, m, kWave);
            a1 += __shfl_xor(a1, m, kWave);
        }
        if (lane == 0) dist[row] = metric == OGS_KMEANS_WIDE_L2 ? a0 : (a1 > 0.f ? 1.f - a0 / sqrtf(a1) : 1.f);
    }
}

__global__ __launch_bounds__(kBlock) void wide_ones_kernel(float* __restrict__ p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) p[i] = 1.f;
}

// One wave per centre: centre = sums / wsum (cosine: then normalised, the norm in fp64 so that the result is a unit vector to
// one rounding per element); wsum == 0, or a zero norm under cosine, keeps the previous bytes.  counts = wsum.
__global__ __launch_bounds__(kBlock) void wide_finalize_kernel(const float* __restrict__ sums, const float* __restrict__ wsum, int k,
                                                               int D, int metric, float* __restrict__ C, float* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (c >= k) return;
    const float ws = wsum[c];
    if (counts && lane == 0) counts[c] = ws;
    if (!(ws > 0.f)) return;
    const float* s = sums + (int64_t)c * D;
    float* out = C + (int64_t)c * D;
    if (metric == OGS_KMEANS_WIDE_L2) {
        for (int d = lane; d < D; d += kWave) out[d] = s[d] / ws;
        return;
    }
    double n2 = 0.0;
    for (int d = lane; d < D; d += kWave) {
        const double v = (double)(s[d] / ws);
        n2 += v * v;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) n2 += __shfl_xor(n2, m, kWave);
    if (!(n2 > 0.0)) return;
    const double n = sqrt(n2);
    for (int d = lane; d < D; d += kWave) out[d] = (float)((double)(s[d] / ws) / n);
}

// sum w dist in fp64: every thread a strided chain, a tree per workgroup, then one workgroup over the partials -- the order is a
// function of N alone
__device__ __forceinline__ double block_tree_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int m = kBlock / 2; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) sh[threadIdx.x] += sh[threadIdx.x + m];
        __syncthreads();
    }
    return sh[0];
}
__global__ __launch_bounds__(kBlock) void wide_inertia_kernel(const float* __restrict__ dist, const float* __restrict__ w, int64_t N,
                                                              double* __restrict__ partials) {
    __shared__ double sh[kBlock];
    double a = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += (int64_t)gridDim.x * kBlock)
        a += (w ? (double)w[i] : 1.0) * (double)dist[i];
    const double t = block_tree_sum(a, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
__global__ __launch_bounds__(kBlock) void wide_inertia_total_kernel(const double* __restrict__ partials, int nb, double* __restrict__ total) {
    __shared__ double sh[kBlock];
    const double t = block_tree_sum((int)threadIdx.x < nb ? partials[threadIdx.x] : 0.0, sh);
    if (threadIdx.x == 0) total[0] = t;
}

// ---- host side ------------------------------------------------------------------------------------------------------------
bool wide_sizes_ok(int64_t N, int D, int k) {
    return N >= 0 && N < ((int64_t)1 << 31) && D >= 1 && D <= kWideMaxDim && k >= 1 && k <= kWideMaxK;
}
int pad_dim(int D) { return (D + kDimStep - 1) / kDimStep * kDimStep; }
// 16-row sub-tiles whose planes (6 B per element) fit in LDS: 4 up to D = 384, 3 up to 512, 2 up to 768, 1 beyond.
// -DOGS_KMEANS_WIDE_MAX_NT=1|2|3 and -DOGS_KMEANS_WIDE_THREADS=256|512|1024 (build.py --variant) pin the tile and the workgroup:
// the A-B behind both choices
#ifndef OGS_KMEANS_WIDE_MAX_NT
#define OGS_KMEANS_WIDE_MAX_NT 4
#endif
size_t planes_lds(int NT, int Dpad) { return (size_t)NT * 16 * Dpad * 6; }
int wide_row_tiles(int Dpad) {
    int nt = min(OGS_KMEANS_WIDE_MAX_NT, kRowTile / 16);
    while (nt > 1 && planes_lds(nt, Dpad) > kPlanesLds) --nt;
    return nt;
}
// The waves of a workgroup share its row planes and take the centre tiles round robin.  Small planes leave room for several
// workgroups per CU and 4 waves each are enough (more only lengthen the merge); when one or two workgroups fill the LDS, the
// waves that hide the latency of the centre loads have to come from inside the workgroup.
int wide_threads(size_t lds) {
#ifdef OGS_KMEANS_WIDE_THREADS
    return OGS_KMEANS_WIDE_THREADS;
#else
    return lds <= 40 * 1024 ? 256 : (lds <= 80 * 1024 ? 512 : 1024);
#endif
}
int inertia_blocks(int64_t N) { return (int)max((int64_t)1, min((int64_t)kInertiaBlocks, (N + 4 * kBlock - 1) / (4 * kBlock))); }

struct WideTmp {
    float* mu;            // [kWideMaxDim] the L2 shift, zero padded
    u32x4* planes;        // one stage of packed centres
    float* bias;          // [stage]
    float* best;          // [N] best score across stages
    float* dist;          // [N] when the caller keeps no distances but wants the inertia
    float* ones;          // [N]
    int32_t* begin;       // [k + 1]
    int32_t* slots;       // [N]
    float* sums;          // [k, D]
    float* wsum;          // [k]
    double* partials;     // [kInertiaBlocks]
    void* ttmp;           // ogs_knn_transpose
    void* atmp;           // ogs_knn_aggregate_t
    size_t ttmp_bytes, atmp_bytes, bytes;
    static WideTmp carve(void* p, int64_t N, int D, int k) {
        Carver c(p);
        WideTmp t;
        const int stage = min((k + kCentreTile - 1) / kCentreTile * kCentreTile, kStage);
        t.mu = c.take<float>(kWideMaxDim);
        t.partials = c.take<double>(kInertiaBlocks);      // in front of everything sized by D and k: ogs_kmeans_wide_inertia knows neither
        t.planes = c.take<u32x4>((size_t)stage * pad_dim(D) * 6 / sizeof(u32x4));
        t.bias = c.take<float>(stage);
        t.best = c.take<float>(N);
        t.dist = c.take<float>(N);
        t.ones = c.take<float>(N);
        t.begin = c.take<int32_t>((size_t)k + 1);
        t.slots = c.take<int32_t>(N);
        t.sums = c.take<float>((size_t)k * D);
        t.wsum = c.take<float>(k);
        t.ttmp_bytes = ogs_knn_transpose_tmp_bytes(N, 1, k);
        t.atmp_bytes = max(ogs_knn_aggregate_t_tmp_bytes(N, 1, k, D), ogs_knn_aggregate_t_tmp_bytes(N, 1, k, 1));
        t.ttmp = c.take<char>(t.ttmp_bytes);
        t.atmp = c.take<char>(t.atmp_bytes);
        t.bytes = c.off;
        return t;
    }
};

int bad_metric(const char* what, int metric) {
    if (metric == OGS_KMEANS_WIDE_L2 || metric == OGS_KMEANS_WIDE_COSINE) return 0;
    set_error("%s: unknown metric %d", what, metric);
    return 1;
}
int bad_sizes(const char* what, int64_t N, int D, int k) {
    if (wide_sizes_ok(N, D, k)) return 0;
    set_error("%s: bad sizes (N=%lld D=%d k=%d; N < 2^31, 1 <= D <= %d, 1 <= k <= %d)", what, (long long)N, D, k, kWideMaxDim, kWideMaxK);
    return 1;
}
int bad_tmp(const char* what, const void* tmp, size_t have, size_t need) {
    if (tmp && have >= need && (reinterpret_cast<uintptr_t>(tmp) & 15u) == 0) return 0;
    set_error("%s: tmp (16-byte aligned) has %zu bytes, %zu needed (ogs_kmeans_wide_tmp_bytes)", what, tmp ? have : (size_t)0, need);
    return 1;
}

template <int NT>
int launch_score(int64_t N, int D, int KC, const WideTmp& t, int nct, int c0, bool first, bool last, int metric, const float* X,
                 const float* C, int32_t* ids, float* dist, hipStream_t s) {
    constexpr int RT = NT * 16;
    const size_t planes = planes_lds(NT, KC * kDimStep);
    const int threads = wide_threads(planes);
    const size_t lds = max(planes, (size_t)RT * (4 * threads / kWave) * 8 + (size_t)RT * 4);      // the merge table reuses the planes
    if (lds > 160 * 1024) { set_error("kmeans_wide: %zu bytes of LDS requested (> 160 KiB)", lds); return OGS_ERR_UNSUPPORTED; }
    if (lds > 48 * 1024)
        OGS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(wide_score_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned nb = (unsigned)((N + RT - 1) / RT);
    OGS_LAUNCH_NAMED("wide_score_kernel", (wide_score_kernel<NT>), dim3(nb), dim3(threads), lds, s, X, N, D, KC,
                     (const u32x4*)t.planes, (const float*)t.bias, nct, c0, (int)first, (int)last, metric, (const float*)t.mu, C,
                     t.best, ids, dist);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

int wide_assign(const float* X, int64_t N, int D, const float* C, int k, int metric, int32_t* ids, float* dist, const WideTmp& t,
                hipStream_t s) {
    const int Dpad = pad_dim(D), KC = Dpad / kDimStep, NT = wide_row_tiles(Dpad);
    OGS_LAUNCH(wide_shift_kernel, dim3(1), dim3(kBlock), 0, s, X, N, D, Dpad, metric, t.mu);
    OGS_LAUNCH_CHECK(0, s);
    for (int c0 = 0; c0 < k; c0 += kStage) {
        const int nc = min(kStage, k - c0), nct = (nc + kCentreTile - 1) / kCentreTile;
        OGS_LAUNCH(wide_pack_kernel, dim3(nct), dim3(kBlock), 0, s, C, k, D, KC, c0, metric, (const float*)t.mu, t.planes, t.bias);
        OGS_LAUNCH_CHECK(0, s);
        const bool first = c0 == 0, last = c0 + kStage >= k;
        int rc;
        switch (NT) {
            case 4: rc = launch_score<4>(N, D, KC, t, nct, c0, first, last, metric, X, C, ids, dist, s); break;
            case 3: rc = launch_score<3>(N, D, KC, t, nct, c0, first, last, metric, X, C, ids, dist, s); break;
            case 2: rc = launch_score<2>(N, D, KC, t, nct, c0, first, last, metric, X, C, ids, dist, s); break;
            default: rc = launch_score<1>(N, D, KC, t, nct, c0, first, last, metric, X, C, ids, dist, s); break;
        }
        if (rc != OGS_OK) return rc;
    }
    return OGS_OK;
}

int wide_update(const float* X, const float* w, int64_t N, int D, const int32_t* ids, int k, int metric, float* C, float* counts,
                const WideTmp& t, hipStream_t s) {
    void* sv = static_cast<void*>(s);
    OGS_LAUNCH(wide_ones_kernel, dim3((unsigned)((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, t.ones, N);
    OGS_LAUNCH_CHECK(0, s);
    int rc = ogs_knn_transpose(N, 1, k, ids, t.begin, t.slots, t.ttmp, t.ttmp_bytes, sv);
    if (rc != OGS_OK) return rc;
    const float* wv = w ? w : t.ones;
    rc = ogs_knn_aggregate_t(N, 1, k, D, t.begin, t.slots, wv, X, t.sums, t.atmp, t.atmp_bytes, sv);
    if (rc != OGS_OK) return rc;
    rc = ogs_knn_aggregate_t(N, 1, k, 1, t.begin, t.slots, wv, t.ones, t.wsum, t.atmp, t.atmp_bytes, sv);
    if (rc != OGS_OK) return rc;
    OGS_LAUNCH(wide_finalize_kernel, dim3((unsigned)((k + 3) / 4)), dim3(kBlock), 0, s, (const float*)t.sums, (const float*)t.wsum, k, D,
               metric, C, counts);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

int wide_inertia(const float* dist, const float* w, int64_t N, double* total, const WideTmp& t, hipStream_t s) {
    const int nb = inertia_blocks(N);
    OGS_LAUNCH(wide_inertia_kernel, dim3(nb), dim3(kBlock), 0, s, dist, w, N, t.partials);
    OGS_LAUNCH_CHECK(0, s);
    OGS_LAUNCH(wide_inertia_total_kernel, dim3(1), dim3(kBlock), 0, s, (const double*)t.partials, nb, total);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

}  // namespace
}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_kmeans_wide_row_tile(void) { return kRowTile; }
size_t ogs_kmeans_wide_centre_tile(void) { return kCentreTile; }
size_t ogs_kmeans_wide_dim_step(void) { return kDimStep; }
size_t ogs_kmeans_wide_stage(void) { return kStage; }
size_t ogs_kmeans_wide_max_dim(void) { return kWideMaxDim; }
size_t ogs_kmeans_wide_max_k(void) { return kWideMaxK; }

size_t ogs_kmeans_wide_tmp_bytes(int64_t N, int32_t D, int32_t k) {
    if (!wide_sizes_ok(N, D, k)) return 0;
    return WideTmp::carve(nullptr, N, D, k).bytes;
}

int ogs_kmeans_wide_assign(const float* X, int64_t N, int32_t D, const float* C, int32_t k, int32_t metric, int32_t* ids, float* dist,
                           void* tmp, size_t tmp_bytes, void* stream) {
    if (bad_sizes("kmeans_wide_assign", N, D, k) || bad_metric("kmeans_wide_assign", metric)) return OGS_ERR_INVALID_ARG;
    if (N == 0) return OGS_OK;
    if (!X || !C || !ids) { set_error("kmeans_wide_assign: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    if (bad_tmp("kmeans_wide_assign", tmp, tmp_bytes, WideTmp::carve(nullptr, N, D, k).bytes)) return OGS_ERR_INVALID_ARG;
    return wide_assign(X, N, D, C, k, metric, ids, dist, WideTmp::carve(tmp, N, D, k), static_cast<hipStream_t>(stream));
}

int ogs_kmeans_wide_update(const float* X, const float* w, int64_t N, int32_t D, const int32_t* ids, int32_t k, int32_t metric, float* C,
                           float* counts, void* tmp, size_t tmp_bytes, void* stream) {
    if (bad_sizes("kmeans_wide_update", N, D, k) || bad_metric("kmeans_wide_update", metric)) return OGS_ERR_INVALID_ARG;
    if (!C) { set_error("kmeans_wide_update: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (N == 0) {                                       // every centre is empty and keeps its value
        if (counts) OGS_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)k * sizeof(float), s));
        return OGS_OK;
    }
    if (!X || !ids) { set_error("kmeans_wide_update: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    if (bad_tmp("kmeans_wide_update", tmp, tmp_bytes, WideTmp::carve(nullptr, N, D, k).bytes)) return OGS_ERR_INVALID_ARG;
    return wide_update(X, w, N, D, ids, k, metric, C, counts, WideTmp::carve(tmp, N, D, k), s);
}

int ogs_kmeans_wide_inertia(const float* dist, const float* w, int64_t N, double* total, void* tmp, size_t tmp_bytes, void* stream) {
    if (N < 0 || N >= ((int64_t)1 << 31)) { set_error("kmeans_wide_inertia: bad N=%lld", (long long)N); return OGS_ERR_INVALID_ARG; }
    if (!total || (N > 0 && !dist)) { set_error("kmeans_wide_inertia: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    if (bad_tmp("kmeans_wide_inertia", tmp, tmp_bytes, WideTmp::carve(nullptr, N, 1, 1).bytes)) return OGS_ERR_INVALID_ARG;
    return wide_inertia(dist, w, N, total, WideTmp::carve(tmp, N, 1, 1), static_cast<hipStream_t>(stream));
}

int ogs_kmeans_wide_lloyd(const float* X, const float* w, int64_t N, int32_t D, float* C, int32_t k, int32_t metric, int32_t iters,
                          int32_t* ids, float* dist, float* counts, double* inertia, void* tmp, size_t tmp_bytes, void* stream) {
    if (bad_sizes("kmeans_wide_lloyd", N, D, k) || bad_metric("kmeans_wide_lloyd", metric)) return OGS_ERR_INVALID_ARG;
    if (iters < 0) { set_error("kmeans_wide_lloyd: bad iters=%d", iters); return OGS_ERR_INVALID_ARG; }
    if (!C || (N > 0 && (!X || !ids))) { set_error("kmeans_wide_lloyd: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    if (bad_tmp("kmeans_wide_lloyd", tmp, tmp_bytes, WideTmp::carve(nullptr, N, D, k).bytes)) return OGS_ERR_INVALID_ARG;
    const WideTmp t = WideTmp::carve(tmp, N, D, k);
    float* dv = dist ? dist : (inertia ? t.dist : nullptr);
    for (int it = 0; it <= iters; ++it) {
        int rc = ogs_kmeans_wide_assign(X, N, D, C, k, metric, ids, dv, tmp, tmp_bytes, stream);
        if (rc == OGS_OK && inertia) rc = ogs_kmeans_wide_inertia(dv, w, N, inertia + it, tmp, tmp_bytes, stream);
        if (rc == OGS_OK && it < iters) rc = ogs_kmeans_wide_update(X, w, N, D, ids, k, metric, C, counts, tmp, tmp_bytes, stream);
        if (rc != OGS_OK) return rc;
    }
    return OGS_OK;
}

}  // extern "C"
