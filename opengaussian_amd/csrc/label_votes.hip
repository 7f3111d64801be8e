// Pixel labels lifted to Gaussians in one walk of a finished pass (include/ogs_query.h: ogs_raster_label_votes).
//
// The transpose of label_map.hip: there every Gaussian carries a label and every pixel gets the label it shows; here every pixel
// carries a label and every Gaussian (or the row it is mapped to) gets, per label, the blend weight w_i(p) = alpha_i * T_i it puts
// on the pixels of that label, seen through the occlusion of the whole pass:
//     votes[row(g), l] += sum over the pixels p with lab(p) = l of w_{entry of g}(p)            int64, quantum 2^-32
// One workgroup per tile, wave = 8x8 quadrant, lane = pixel, the quadrant's stream 64 entries at a time with the records parked
// in LDS and broadcast, T / done / the stop rule per lane: the walk of label_map_kernel, restated with the same arithmetic
// (blend_power, |power + h| <= h, min(0.99, opacity * __expf(power)), the 1/255 skip, the stop at T * (1 - alpha) < 1e-4; this
// file is compiled with -ffp-contract=off).
//
// What is new is the per-entry reduction over the wave's 64 pixels, grouped by the pixel's label.  The labels of the 64 pixels
// are known before the walk: the wave builds its local dictionary once (first occurrence in lane order; K <= 64 distinct
// values, typically 1-3) and every pixel keeps its local index.  Entries that put weight on the quadrant and map to a counted
// row are staged sixteen at a time (one ds_write of the 64 weights each); the batch is then folded on the matrix pipe as
//     D[16 entries, 16 local labels] = Wt[16, 64 pixels] x OneHot[64, 16]          v_mfma_f32_16x16x4_f32, exact fp32
// (the fold of the features-only backward, RankOneFold in blend_bwd.hip, with the one-hot of the pixel's local index in place
// of the upstream gradient).  A quadrant with more than 16 local labels takes ceil(K / 16) column blocks over the same staged
// A tile, so any quadrant is done in ONE walk.
//
// A partial -- one entry, one quadrant, one label -- is therefore the fp32 value
//     (chain over even j of its pixels 4 j + k, k = 0..3) + (chain over odd j), every chain an fma(w, 1, acc) from +0 in pixel
//     order, the pixels of other labels entering as fma(w, 0, acc) = acc
// a function of the weights of that label's pixels and of their lane positions only: not of the label's value, of its local
// index, of its column block or of the other labels of the quadrant.  The partial is rounded ONCE, __float2ll_rn(partial * 2^32)
// (the rule of the group statistics, kFixedScale in blend_fwd.hip), and added to its cell with an integer atomic from the
// vector lanes; integer addition commutes, so two runs give the same bytes and V views sum into one table.
//
// The four quadrants of a tile are NOT merged in LDS before the atomics: a cell is (row, label), four quadrants of a tile share
// a cell only where they share a label, and DESIGN section 3b measured such merges slower than the atomics they save.
#include "ogs_common.h"
#include "../../include/ogs_query.h"

namespace ogs {
namespace {

constexpr float kAlphaMin = 1.0f / 255.0f;
constexpr float kVoteScale = 4294967296.0f;          // 2^32, kFixedScale of the group statistics
constexpr int kWaves = kBlock / kWave;
constexpr int kFoldRows = 16;                        // entries per batch: rows of the A tile
constexpr int kFoldCols = 16;                        // local labels per column block: columns of the B tile
constexpr int kFoldStride = 66;                      // row stride in words: the transposed read is bank-conflict free
typedef float floatx4 __attribute__((ext_vector_type(4)));
// Timing ablations (scripts/label_votes_bench.py: where the time goes).  The results are WRONG by construction, so the switches
// exist only in a -DOGS_EXPERIMENTS variant build; the shipped library compiles both to `false`.  Each gates its step on a
// value that never occurs (a weight sum of -1, T = -1), so the compiler keeps everything in front of the step.
#if defined(OGS_EXPERIMENTS) && defined(OGS_VOTES_WALK_ONLY)
constexpr bool kSkipFold = true;                     // the walk alone: nothing is staged, folded or added
#else
constexpr bool kSkipFold = false;
#endif
#if defined(OGS_EXPERIMENTS) && defined(OGS_VOTES_NO_ATOMICS)
constexpr bool kSkipAtomics = true;                  // walk, staging and fold; no cell is added
#else
constexpr bool kSkipAtomics = false;
#endif

struct VotesLds {
    float4 rec[kWaves][kWave * 2];                   // per wave: geometry of the 64 entries of a sub-chunk
    int32_t row[kWaves][kWave];                      // per wave: table row of each of them, -1 = not counted
    float w[kWaves][kFoldRows * kFoldStride];        // per wave: the weights of the staged entries, [entry][pixel]
    int32_t dict[kWaves][kWave];                     // per wave: label of each local index
    int32_t lidx[kWaves][kWave];                     // per wave: local index of each pixel, -1 outside the image
};

__global__ __launch_bounds__(kBlock) void label_votes_kernel(
    const uint2* __restrict__ ranges, const uint32_t* __restrict__ qcount, const float* __restrict__ stream, int RS,
    const uint32_t* __restrict__ quad_list, int W, int H, int gx, int tiles, const uint32_t* __restrict__ tile_order, int P,
    const int32_t* __restrict__ pixel_labels, int L, const int32_t* __restrict__ rows_of, int R,
    unsigned long long* __restrict__ votes) {
    __shared__ VotesLds lds;
    const int tile = tile_order ? (int)tile_order[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)tile >= (unsigned)tiles) return;            // block-uniform; an order the pass never wrote addresses nothing
    const int tx = tile % gx, ty = tile / gx;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int px = tx * kTile + (wave & 1) * 8 + (lane & 7);
    const int py = ty * kTile + (wave >> 1) * 8 + (lane >> 3);
    const bool inside = px < W && py < H;
    const float fx = (float)px, fy = (float)py;

    // both layouts with one formula (label_map_kernel): the tile owns n_tile slots at range.x, of which it packed n_kept
    const uint2 range = ranges[tile];
    const int n_tile = (int)(range.y - range.x);
    const int n = min((int)qcount[tile * 5 + wave], n_tile), n_kept = min((int)qcount[tile * 5 + 4], n_tile);
    if (n <= 0) return;                                       // wave-uniform; no workgroup barrier follows
    const float* __restrict__ tb = stream + (size_t)range.x * RS;
    const uint32_t* __restrict__ qi = quad_list + ((size_t)range.x * 5 + (size_t)wave * n_tile);
    const uint32_t lim = n_kept > 0 ? (uint32_t)n_kept - 1u : 0u;

    float4* __restrict__ recs = lds.rec[wave];
    int32_t* __restrict__ rows = lds.row[wave];
    float* __restrict__ wbuf = lds.w[wave];
    int32_t* __restrict__ dict = lds.dict[wave];

    // ---- the quadrant's local dictionary: first occurrence in lane order --------------------------------------------------------
    int32_t lab = L;
    if (inside) {
        const int32_t l = pixel_labels[(size_t)py * W + px];
        lab = (l >= 0 && l < L) ? l : L;                      // column L: no label
    }
    int32_t my_idx = -1;
    int K = 0;
    for (unsigned long long left = __ballot(inside); left != 0ull; ++K) {          // wave-uniform
        const int leader = __ffsll((long long)left) - 1;
        const int32_t v = __shfl(lab, leader, kWave);
        const bool mine = inside && lab == v;
        if (mine) my_idx = K;
        if (lane == leader) dict[K] = v;
        left &= ~__ballot(mine);
    }
    lds.lidx[wave][lane] = my_idx;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int m = lane & 15, kq = lane >> 4;                  // operand row / column, k group
    int32_t li[16];                                           // local index of pixel 4 j + kq: the B tile, loop invariant
#pragma unroll
    for (int j = 0; j < 16; ++j) li[j] = lds.lidx[wave][4 * j + kq];
    const int nblk = (K + kFoldCols - 1) / kFoldCols;

    int cnt = 0;                                              // wave-uniform: entries staged
    int32_t rowv = -1;                                        // lane e: table row of staged entry e
    const int64_t pitch = (int64_t)L + 1;

    auto flush = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        float a[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) a[j] = m < cnt ? wbuf[m * kFoldStride + 4 * j + kq] : 0.f;
        for (int cb = 0; cb < nblk; ++cb) {
            const int col = cb * kFoldCols + m;
            floatx4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = d0;
#pragma unroll
            for (int j = 0; j < 16; j += 2) {
                d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], li[j] == col ? 1.f : 0.f, d0, 0, 0, 0);
                d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j + 1], li[j + 1] == col ? 1.f : 0.f, d1, 0, 0, 0);
            }
            const floatx4 d = d0 + d1;
            const int32_t label = col < K ? dict[col] : -1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = 4 * kq + r;
                const int32_t row = __shfl(rowv, e, kWave);
                // every index checked where it is used: a staged row lies in [0, R), a dictionary label in [0, L]
                if (e < cnt && d[r] != 0.f && (uint32_t)row < (uint32_t)R && label >= 0 && label <= L &&
                    (!kSkipAtomics || d[r] == -1.f))
                    atomicAdd(votes + ((size_t)row * (size_t)pitch + (size_t)label),
                              (unsigned long long)__float2ll_rn(d[r] * kVoteScale));
            }
        }
        cnt = 0;
        __builtin_amdgcn_wave_barrier();                      // the staging may be rewritten
    };

    // ---- the quadrant's stream, 64 entries at a time ------------------------------------------------------------------------------
    float T = 1.0f;
    bool done = !inside;
    for (int c0 = 0; c0 < n && __ballot(!done) != 0ull; c0 += kWave) {
        const int chunk = min(kWave, n - c0);
        if (lane < chunk) {
            const uint32_t ridx = min(qi[c0 + lane], lim);
            const float4* __restrict__ rp = reinterpret_cast<const float4*>(tb + (size_t)ridx * RS);
            const float4 g0 = rp[0], g1 = rp[1];
            const uint32_t id = __float_as_uint(g1.w);
            int32_t row = -1;
            if (id < (uint32_t)P) {
                const int32_t r = rows_of ? rows_of[id] : (int32_t)id;
                if (r >= 0 && r < R) row = r;                 // outside [0, R): occludes, is not counted
            }
            recs[lane * 2] = g0;
            recs[lane * 2 + 1] = g1;
            rows[lane] = row;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int e = 0; e < chunk && __ballot(!done) != 0ull; ++e) {
            const float4 g0 = recs[e * 2], g1 = recs[e * 2 + 1];             // x y a2 c2 | b2 h opacity id
            const float dx = g0.x - fx, dy = g0.y - fy;
            const float power = blend_power(g0.z, g1.x, g0.w, dx, dy);
            const bool cand = !done && fabsf(power + g1.y) <= g1.y;
            if (__ballot(cand) == 0ull) continue;
            const float araw = fminf(0.99f, g1.z * __expf(power));
            const bool act = cand && araw >= kAlphaMin;
            const float alpha = act ? araw : 0.f;
            const float test_T = T * (1.0f - alpha);
            const bool stop = test_T < 0.0001f;
            const float w = stop ? 0.f : alpha * T;
            T = stop ? T : test_T;
            done = done || stop;
            const int32_t row = __builtin_amdgcn_readfirstlane(rows[e]);     // the same word in every lane
            if (row >= 0 && __ballot(w != 0.f) != 0ull && (!kSkipFold || T == -1.f)) {
                wbuf[cnt * kFoldStride + lane] = w;
                if (lane == cnt) rowv = row;
                if (++cnt == kFoldRows) flush();
            }
        }
        __builtin_amdgcn_wave_barrier();                                     // the record staging may be rewritten
    }
    if (cnt > 0) flush();
}

}  // namespace
}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_label_votes_quadrant_capacity(void) { return (size_t)kWave; }
size_t ogs_label_votes_fold_columns(void) { return (size_t)kFoldCols; }

int ogs_raster_label_votes(const OgsRasterFwdArgs* a, const OgsLabelVotesArgs* lv, void* stream_) {
    if (!a || !lv) { set_error("label_votes: args == NULL"); return OGS_ERR_INVALID_ARG; }
    if (a->P <= 0 || a->W <= 0 || a->H <= 0) { set_error("label_votes: bad sizes P=%d W=%d H=%d", a->P, a->W, a->H); return OGS_ERR_INVALID_ARG; }
    if (a->C != 3 && a->C != 6 && a->C != 9 && a->C != 12) { set_error("C=%d unsupported (3, 6, 9, 12)", a->C); return OGS_ERR_UNSUPPORTED; }
    if (a->num_groups > 1) { set_error("label_votes: grouped passes are not supported"); return OGS_ERR_UNSUPPORTED; }
    if (lv->num_labels < 0) { set_error("label_votes: num_labels=%d", lv->num_labels); return OGS_ERR_INVALID_ARG; }
    if (lv->num_rows < 1) { set_error("label_votes: num_rows=%d", lv->num_rows); return OGS_ERR_INVALID_ARG; }
    if (!a->image_buffer || !a->sorted_rec || !a->quad_list || !lv->pixel_labels || !lv->votes) {
        set_error("label_votes: NULL required pointer (image_buffer, sorted_rec, quad_list, pixel_labels, votes)");
        return OGS_ERR_INVALID_ARG;
    }
    const ImageState is = ImageState::carve(a->image_buffer, a->W, a->H, 1);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int gx = (a->W + kTile - 1) / kTile, gy = (a->H + kTile - 1) / kTile;
    const int tiles = gx * gy;
    const uint32_t* order = tile_order_of(is, tiles, a->P);        // heaviest first, as the kept pass ran
    OGS_LAUNCH(label_votes_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, s, (const uint2*)is.ranges, (const uint32_t*)is.qcount,
               (const float*)a->sorted_rec, stream_vec4(a->C) * 4, (const uint32_t*)quad_base(a->quad_list), a->W, a->H, gx, tiles,
               order, a->P, lv->pixel_labels, lv->num_labels, lv->rows, lv->num_rows, (unsigned long long*)lv->votes);
    OGS_LAUNCH_CHECK(a->debug, s);
    return OGS_OK;
}

}  // extern "C"
