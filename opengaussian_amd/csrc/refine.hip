// Multi-view SAM mask refinement as batched footprint kernels (include/ogs_refine.h).
//
// The reference (utils/sam_refinement_utils.py:1118-1318) renders one white Gaussian per rasterizer call for every
// (Gaussian, camera) pair.  Here a pair is a walk over the Gaussian's tile rectangle that evaluates the conic the geometry
// phase of the camera left in geom_buffer -- the same record row, the same blend_power / __expf arithmetic as the blend
// kernels (this file is compiled with -ffp-contract=off), so q below is bit for bit the uint8 pixel of a P = 1 pass.
#include "ogs_common.h"
#include "../../include/ogs_refine.h"

namespace ogs {
namespace {

constexpr float kAlphaMin = 1.0f / 255.0f;
// the white SH of render_single_gaussian(use_view_inv_white_shs=True): SH_C0 * 1 + 0.5, as sh_to_rgb rounds it
constexpr float kWhite = 0.28209479177387814f * 1.0f + 0.5f;
constexpr int kWaveTable = 512;                 // label slots per wave (dense index or open addressing)
constexpr int kWaveMaxPixels = 64 * 64;         // 64 rounds of one wave; larger rectangles take a workgroup
constexpr int kBlockTable = 4096;               // dense label slots of the workgroup-per-pair kernel (16 KB of LDS)
constexpr int kWavesPerBlock = kBlock / kWave;

struct Foot {
    float px, py, a2, b2, c2, h, op;
    int x0, y0, w, hgt;                         // pixel rectangle: the tile rectangle clipped to the image
};

// false: culled by the geometry phase (radius 0) or an empty rectangle -- nothing is drawn
__device__ __forceinline__ bool load_foot(const float4* __restrict__ rec, int recv4, int g, int W, int H, Foot& f) {
    const float4 a = rec[(size_t)g * recv4], b = rec[(size_t)g * recv4 + 1];
    const int radius = __float_as_int(a.w);
    if (radius <= 0) return false;
    const int gx = (W + kTile - 1) / kTile, gy = (H + kTile - 1) / kTile;
    const float rf = (float)radius;
    auto tr = [](float v) -> int {
        if (!(fabsf(v) < 3.0e38f)) v = 0.f;
        v = fminf(fmaxf(v, -2.0e9f), 2.0e9f);
        return (int)v;
    };
    // same expressions as preprocess_one step 8 / tiny_blend_kernel
    const int rminx = min(gx, max(0, tr((a.x - rf) / (float)kTile)));
    const int rminy = min(gy, max(0, tr((a.y - rf) / (float)kTile)));
    const int rmaxx = min(gx, max(0, tr((a.x + rf + (float)kTile - 1.0f) / (float)kTile)));
    const int rmaxy = min(gy, max(0, tr((a.y + rf + (float)kTile - 1.0f) / (float)kTile)));
    f.x0 = rminx * kTile;
    f.y0 = rminy * kTile;
    f.w = min(rmaxx * kTile, W) - f.x0;
    f.hgt = min(rmaxy * kTile, H) - f.y0;
    if (f.w <= 0 || f.hgt <= 0) return false;
    f.px = a.x; f.py = a.y;
    f.a2 = -0.5f * b.x; f.b2 = -b.y; f.c2 = -0.5f * b.z;
    f.h = 0.5f * (__logf(255.0f * b.w) + kThrMargin);      // the blend loops' candidate window: thr <= power <= 0
    f.op = b.w;
    return true;
}

// the uint8 pixel fix_image() makes of the P = 1 render at (x, y)
__device__ __forceinline__ int foot_q(const Foot& f, int x, int y) {
    const float dx = f.px - (float)x, dy = f.py - (float)y;
    const float power = blend_power(f.a2, f.b2, f.c2, dx, dy);
    if (!(fabsf(power + f.h) <= f.h)) return 0;
    const float alpha = fminf(0.99f, f.op * __expf(power));
    if (!(alpha >= kAlphaMin)) return 0;
    const float colour = kWhite * alpha;                   // T = 1, black background
    return (int)fminf(fmaxf(colour * 255.0f, 0.f), 255.f);
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m, kWave), hi = __shfl_xor((uint32_t)(v >> 32), m, kWave);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
    for (int m = kWave / 2; m >= 1; m >>= 1) { const uint64_t o = shfl_xor_u64(v, m); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
    for (int m = kWave / 2; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, kWave));
    return v;
}
// (sum, label) -> one key whose maximum is the largest sum, the lowest label among equals; sum 0 never wins
__device__ __forceinline__ uint64_t vote_key(uint32_t sum, int label) {
    return ((uint64_t)sum << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)label);
}
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(kBlock) void refine_visibility_kernel(
    int P, const float* __restrict__ means3D, const float* __restrict__ view, const float* __restrict__ proj,
    const float* __restrict__ campos, int W, int H, float cx, float cy, const float* __restrict__ depth_map,
    float dist_optical, float depth_thr, uint8_t* __restrict__ visible) {
    const int g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= P) return;
    float V[16], M[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { V[i] = view[i]; M[i] = proj[i]; }
    const float x = means3D[3 * g], y = means3D[3 * g + 1], z = means3D[3 * g + 2];
    float pc[4], cl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) pc[r] = V[4 * r] * x + V[4 * r + 1] * y + V[4 * r + 2] * z + V[4 * r + 3];
#pragma unroll
    for (int r = 0; r < 4; ++r) cl[r] = M[4 * r] * pc[0] + M[4 * r + 1] * pc[1] + M[4 * r + 2] * pc[2] + M[4 * r + 3] * pc[3];
    float w = cl[3];
    if (fabsf(w) < 1e-8f) w = (w > 0.f ? 1e-8f : (w < 0.f ? -1e-8f : 0.f));
    const float u = (cl[0] / w) * ((float)W / 2.0f) + cx;
    const float v = (cl[1] / w) * ((float)H / 2.0f) + cy;
    bool vis = pc[2] > 0.f && u >= 0.f && u < (float)W && v >= 0.f && v < (float)H;     // NaN compares false
    if (vis) {
        const int ui = min((int)u, W - 1), vi = min((int)v, H - 1);
        const float ex = x - campos[0], ey = y - campos[1], ez = z - campos[2];
        const float dist = sqrtf(ex * ex + ey * ey + ez * ez) - dist_optical;
        vis = fabsf(dist - depth_map[(size_t)vi * W + ui]) < depth_thr;
    }
    visible[g] = vis ? 1 : 0;
}

// One wave per pair.  The wave's table is indexed by the label when K fits, else it is an open-addressing table of the
// labels the footprint meets (linear probing; a full table defers the pair to the workgroup kernel).
__global__ __launch_bounds__(kBlock) void refine_footprint_wave_kernel(
    int n_pairs, const int32_t* __restrict__ pairs, const float4* __restrict__ rec, int recv4, int W, int H,
    const int32_t* __restrict__ labels, int K, int32_t* __restrict__ dominant, int32_t* __restrict__ q_max) {
    __shared__ int32_t s_key[kWavesPerBlock][kWaveTable];
    __shared__ uint32_t s_sum[kWavesPerBlock][kWaveTable];
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int i = blockIdx.x * kWavesPerBlock + wave;
    if (i >= n_pairs) return;                              // wave-uniform; no workgroup barrier below
    Foot f;
    if (!load_foot(rec, recv4, pairs[i], W, H, f)) {
        if (lane == 0) { dominant[i] = -1; q_max[i] = 0; }
        return;
    }
    const int npix = f.w * f.hgt;
    if (npix > kWaveMaxPixels) {
        if (lane == 0) dominant[i] = OGS_REFINE_DEFER_LARGE;
        return;
    }
    const bool dense = K <= kWaveTable;
    int32_t* key = s_key[wave];
    uint32_t* sum = s_sum[wave];
    for (int s = lane; s < kWaveTable; s += kWave) { key[s] = -1; sum[s] = 0u; }
    wave_lds_fence();
    int qm = 0;
    bool full = false;
    for (int p = lane; p < npix; p += kWave) {
        const int yy = p / f.w, xx = p - yy * f.w;
        const int x = f.x0 + xx, y = f.y0 + yy;
        const int q = foot_q(f, x, y);
        if (q <= 0) continue;
        qm = max(qm, q);
        const int lab = labels[(size_t)y * W + x];
        if ((uint32_t)lab >= (uint32_t)K) continue;
        if (dense) {
            atomicAdd(&sum[lab], (uint32_t)q);
        } else {
            uint32_t slot = ((uint32_t)lab * 2654435761u) >> (32 - 9);
            static_assert(kWaveTable == 1 << 9, "hash shift");
            bool placed = false;
            for (int probe = 0; probe < kWaveTable; ++probe) {
                int32_t k = key[slot];
                if (k == -1) k = atomicCAS(&key[slot], -1, lab);
                if (k == -1 || k == lab) { atomicAdd(&sum[slot], (uint32_t)q); placed = true; break; }
                slot = (slot + 1) & (kWaveTable - 1);
            }
            full = full || !placed;
        }
    }
    if (__ballot(full) != 0ull) {
        if (lane == 0) dominant[i] = OGS_REFINE_DEFER_TABLE;
        return;
    }
    wave_lds_fence();
    uint64_t best = 0;
    for (int s = lane; s < kWaveTable; s += kWave) {
        const uint32_t v = sum[s];
        const int lab = dense ? s : key[s];
        if (v != 0u) { const uint64_t c = vote_key(v, lab); best = c > best ? c : best; }
    }
    best = wave_max_u64(best);
    qm = wave_max_i32(qm);
    if (lane == 0) {
        q_max[i] = qm;
        dominant[i] = (best >> 32) != 0 ? (int32_t)(0xFFFFFFFFu - (uint32_t)best) : -1;
    }
}

// One workgroup per pair: whole-image footprints, and the pairs whose labels overflowed a wave's table.  The table is a
// dense LDS array when K fits, else the pair's zeroed row of `scratch` in global memory.
__global__ __launch_bounds__(kBlock) void refine_footprint_block_kernel(
    int n_pairs, const int32_t* __restrict__ pairs, const float4* __restrict__ rec, int recv4, int W, int H,
    const int32_t* __restrict__ labels, int K, uint32_t* __restrict__ scratch, int32_t* __restrict__ dominant,
    int32_t* __restrict__ q_max) {
    __shared__ uint32_t s_sum[kBlockTable];
    __shared__ uint64_t s_best[kWavesPerBlock];
    __shared__ int s_qm[kWavesPerBlock];
    const int i = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    if (i >= n_pairs) return;
    Foot f;
    if (!load_foot(rec, recv4, pairs[i], W, H, f)) {       // workgroup-uniform
        if (tid == 0) { dominant[i] = -1; q_max[i] = 0; }
        return;
    }
    const bool in_lds = K <= kBlockTable;
    uint32_t* sum = in_lds ? s_sum : scratch + (size_t)i * K;
    if (in_lds) for (int s = tid; s < K; s += kBlock) s_sum[s] = 0u;
    __syncthreads();
    const int npix = f.w * f.hgt;
    int qm = 0;
    for (int p = tid; p < npix; p += kBlock) {
        const int yy = p / f.w, xx = p - yy * f.w;
        const int x = f.x0 + xx, y = f.y0 + yy;
        const int q = foot_q(f, x, y);
        if (q <= 0) continue;
        qm = max(qm, q);
        const int lab = labels[(size_t)y * W + x];
        if ((uint32_t)lab < (uint32_t)K) atomicAdd(&sum[lab], (uint32_t)q);
    }
    __threadfence();
    __syncthreads();
    uint64_t best = 0;
    for (int s = tid; s < K; s += kBlock) {
        const uint32_t v = in_lds ? s_sum[s] : __hip_atomic_load(&sum[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v != 0u) { const uint64_t c = vote_key(v, s); best = c > best ? c : best; }
    }
    best = wave_max_u64(best);
    qm = wave_max_i32(qm);
    if (lane == 0) { s_best[wave] = best; s_qm[wave] = qm; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kWavesPerBlock; ++w) { best = s_best[w] > best ? s_best[w] : best; qm = max(qm, s_qm[w]); }
        q_max[i] = qm;
        dominant[i] = (best >> 32) != 0 ? (int32_t)(0xFFFFFFFFu - (uint32_t)best) : -1;
    }
}

__global__ __launch_bounds__(kBlock) void refine_vote_kernel(int64_t N, int cams, const int32_t* __restrict__ dominant,
                                                             int32_t* __restrict__ winner) {
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= N) return;
    const int32_t* row = dominant + g * cams;
    int32_t win = OGS_REFINE_NO_VOTE;
    int best = 0;
    for (int c = 0; c < cams; ++c) {
        const int32_t id = row[c];
        if (id == OGS_REFINE_NO_VOTE) continue;
        int votes = 0;
        bool first = true;
        for (int d = 0; d < cams; ++d) {
            if (row[d] == id) { if (d < c) first = false; ++votes; }
        }
        if (first && votes > best) { best = votes; win = id; }     // strictly more: the id met first keeps a tie
    }
    winner[g] = win;
}

template <int G>     // lanes per pair: one wave or the workgroup
__global__ __launch_bounds__(kBlock) void refine_expand_kernel(
    int n_pairs, const int32_t* __restrict__ pairs, const int32_t* __restrict__ win, const int32_t* __restrict__ q_max,
    const float4* __restrict__ rec, int recv4, int W, int H, const int32_t* __restrict__ labels, int K,
    float* __restrict__ acc, int32_t* __restrict__ base) {
    const int i = blockIdx.x * (kBlock / G) + threadIdx.x / G, t = threadIdx.x % G;
    if (i >= n_pairs) return;
    const int k = win[i], qm = q_max[i];
    if ((uint32_t)k >= (uint32_t)K || qm <= 0) return;
    if (t == 0) atomicAdd(&base[k], 1);
    Foot f;
    if (!load_foot(rec, recv4, pairs[i], W, H, f)) return;
    const float wmax = (float)qm / 255.0f;
    const int npix = f.w * f.hgt;
    for (int p = t; p < npix; p += G) {
        const int yy = p / f.w, xx = p - yy * f.w;
        const int x = f.x0 + xx, y = f.y0 + yy;
        const int q = foot_q(f, x, y);
        if (q <= 0) continue;
        const size_t pix = (size_t)y * W + x;
        if (labels[pix] == k) continue;
        atomicAdd(&acc[pix * (size_t)K + k], ((float)q / 255.0f) / wmax);
    }
}

__global__ __launch_bounds__(kBlock) void refine_finalize_kernel(int64_t HW, int K, const int32_t* __restrict__ labels,
                                                                 const float* __restrict__ acc,
                                                                 const int32_t* __restrict__ base, int void_index,
                                                                 float threshold, int32_t* __restrict__ out) {
    const int64_t pix = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (pix >= HW) return;
    const int lab = labels[pix];
    const float* row = acc + (size_t)pix * K;
    float best = -1.f;
    int arg = -1;
    for (int k = 0; k < K; ++k) {
        float v = row[k];
        if (k == lab) v = ((k == void_index ? 0.f : 1.f) + (float)base[k]) + v;
        if (v > best) { best = v; arg = k; }
    }
    out[pix] = best < threshold ? -1 : arg;
}

int check_pairs(const char* what, int n_pairs, const void* pairs, const void* geom, int C, int W, int H, const void* labels,
                int K) {
    if (n_pairs < 0 || W <= 0 || H <= 0 || K <= 0 || C <= 0) {
        set_error("%s: bad sizes (n_pairs=%d W=%d H=%d K=%d C=%d)", what, n_pairs, W, H, K, C);
        return OGS_ERR_INVALID_ARG;
    }
    if (n_pairs > 0 && (!pairs || !geom || !labels)) { set_error("%s: NULL pointer", what); return OGS_ERR_INVALID_ARG; }
    return OGS_OK;
}

}  // namespace
}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_refine_wave_table_capacity(void) { return kWaveTable; }
size_t ogs_refine_wave_max_pixels(void) { return kWaveMaxPixels; }
size_t ogs_refine_block_scratch_words(int32_t K) { return K > kBlockTable ? (size_t)K : 0; }

int ogs_refine_visibility(int32_t P, const float* means3D, const float* view, const float* proj, const float* campos,
                          int32_t W, int32_t H, float cx, float cy, const float* depth_map, float dist_optical_center,
                          float depth_diff_threshold, uint8_t* visible, void* stream_) {
    if (P < 0 || W <= 0 || H <= 0) { set_error("refine_visibility: bad sizes"); return OGS_ERR_INVALID_ARG; }
    if (P == 0) return OGS_OK;
    if (!means3D || !view || !proj || !campos || !depth_map || !visible) {
        set_error("refine_visibility: NULL pointer"); return OGS_ERR_INVALID_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    OGS_LAUNCH(refine_visibility_kernel, dim3((unsigned)((P + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, P, means3D, view,
               proj, campos, W, H, cx, cy, depth_map, dist_optical_center, depth_diff_threshold, visible);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

int ogs_refine_footprint_labels(int32_t n_pairs, const int32_t* pairs, const void* geom_buffer, int32_t C, int32_t W,
                                int32_t H, const int32_t* labels, int32_t K, int32_t* dominant, int32_t* q_max,
                                void* stream_) {
    int rc = check_pairs("refine_footprint_labels", n_pairs, pairs, geom_buffer, C, W, H, labels, K);
    if (rc != OGS_OK || n_pairs == 0) return rc;
    if (!dominant || !q_max) { set_error("refine_footprint_labels: NULL output"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    OGS_LAUNCH(refine_footprint_wave_kernel, dim3((unsigned)((n_pairs + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock),
               0, s, n_pairs, pairs, static_cast<const float4*>(geom_buffer), rec_vec4(C), W, H, labels, K, dominant, q_max);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

int ogs_refine_footprint_labels_block(int32_t n_pairs, const int32_t* pairs, const void* geom_buffer, int32_t C,
                                      int32_t W, int32_t H, const int32_t* labels, int32_t K, uint32_t* scratch,
                                      int32_t* dominant, int32_t* q_max, void* stream_) {
    int rc = check_pairs("refine_footprint_labels_block", n_pairs, pairs, geom_buffer, C, W, H, labels, K);
    if (rc != OGS_OK || n_pairs == 0) return rc;
    if (!dominant || !q_max || (K > kBlockTable && !scratch)) {
        set_error("refine_footprint_labels_block: NULL output or scratch"); return OGS_ERR_INVALID_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    OGS_LAUNCH(refine_footprint_block_kernel, dim3((unsigned)n_pairs), dim3(kBlock), 0, s, n_pairs, pairs,
               static_cast<const float4*>(geom_buffer), rec_vec4(C), W, H, labels, K, scratch, dominant, q_max);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

int ogs_refine_vote(int64_t N, int32_t cams, const int32_t* dominant, int32_t* winner, void* stream_) {
    if (N < 0 || cams < 0 || N > (int64_t)INT32_MAX * kBlock) { set_error("refine_vote: bad sizes"); return OGS_ERR_INVALID_ARG; }
    if (N == 0) return OGS_OK;
    if (!winner || (cams > 0 && !dominant)) { set_error("refine_vote: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    OGS_LAUNCH(refine_vote_kernel, dim3((unsigned)((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, N, cams, dominant, winner);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

int ogs_refine_expand(int32_t n_pairs, const int32_t* pairs, const int32_t* win, const int32_t* q_max,
                      const void* geom_buffer, int32_t C, int32_t W, int32_t H, const int32_t* labels, int32_t K,
                      float* acc, int32_t* base, int32_t block_per_pair, void* stream_) {
    int rc = check_pairs("refine_expand", n_pairs, pairs, geom_buffer, C, W, H, labels, K);
    if (rc != OGS_OK || n_pairs == 0) return rc;
    if (!win || !q_max || !acc || !base) { set_error("refine_expand: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const float4* rec = static_cast<const float4*>(geom_buffer);
    if (block_per_pair)
        OGS_LAUNCH(refine_expand_kernel<kBlock>, dim3((unsigned)n_pairs), dim3(kBlock), 0, s, n_pairs, pairs, win, q_max, rec,
                   rec_vec4(C), W, H, labels, K, acc, base);
    else
        OGS_LAUNCH(refine_expand_kernel<kWave>, dim3((unsigned)((n_pairs + kWavesPerBlock - 1) / kWavesPerBlock)),
                   dim3(kBlock), 0, s, n_pairs, pairs, win, q_max, rec, rec_vec4(C), W, H, labels, K, acc, base);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

int ogs_refine_finalize(int64_t HW, int32_t K, const int32_t* labels, const float* acc, const int32_t* base,
                        int32_t void_index, float threshold, int32_t* out, void* stream_) {
    if (HW < 0 || K <= 0 || HW > (int64_t)INT32_MAX * kBlock) { set_error("refine_finalize: bad sizes"); return OGS_ERR_INVALID_ARG; }
    if (HW == 0) return OGS_OK;
    if (!labels || !acc || !base || !out) { set_error("refine_finalize: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    OGS_LAUNCH(refine_finalize_kernel, dim3((unsigned)((HW + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, HW, K, labels, acc,
               base, void_index, threshold, out);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

}  // extern "C"
