// Dense feature images lifted to Gaussians in one call over a finished pass (include/ogs_query.h: ogs_raster_feature_votes).
//
// label_votes.hip with a dense B operand: there every pixel carries ONE label and the fold's B tile is the one-hot of it; here
// every pixel carries a vector F[0..D)(p) and every Gaussian (or the row it is mapped to) gets the blend-weighted sum of it,
// together with the weight itself, seen through the occlusion of the whole pass:
//     table[row(g), c] += sum over the pixels p of v(p) * w_{entry of g}(p) * F[c, p]        c < D       int64, quantum 2^-32
//     table[row(g), D] += sum over the pixels p of v(p) * w_{entry of g}(p)
// v(p) = 1 inside the image where `valid` is NULL or non-zero, else 0.  One workgroup per (tile, block of kBlockCols columns),
// wave = 8x8 quadrant, lane = pixel, the quadrant's stream 64 entries at a time with the records parked in LDS and broadcast,
// T / done / the stop rule per lane: the walk of label_votes_kernel, restated with the same arithmetic (blend_power,
// |power + h| <= h, min(0.99, opacity * __expf(power)), the 1/255 skip, the stop at T * (1 - alpha) < 1e-4, w = alpha * T with
// T from before the update; this file is compiled with -ffp-contract=off).  `valid` does not touch the walk: an invalid pixel
// is occluded and occludes as any other, it only contributes to no column.
//
// The fold is the vote kernel's: entries that put weight on the quadrant and map to a counted row are staged sixteen at a time
// (one ds_write of the 64 weights each), then
//     D[16 entries, 16 columns] = Wt[16, 64 pixels] x B[64 pixels, 16 columns]          v_mfma_f32_16x16x4_f32, exact fp32
// sixteen MFMAs in two accumulator chains (even and odd k-steps), pixel 4 j + kq at step j.  B[p, c] = v(p) * F[c, p], v(p)
// for the weight column c = D, 0 beyond it.  A quadrant's B tile for all of D cannot live on chip (D = 512: 128 KB per wave),
// so a wave keeps kBlockCols columns in registers, sixteen VGPRs per 16-column block, loaded once before the walk, and the
// walk is repeated per block of kBlockCols columns along the grid's second dimension: ONE launch for all of D.
//
// A partial -- one entry, one quadrant, one column -- is therefore the fp32 value
//     (chain over even j of fma(w[4 j + k], B[4 j + k, c], acc), k = 0..3, from +0) + (the same chain over odd j)
// a function of that column's 64 B values and of the weights only: not of the column's index, of its 16-column block or of its
// grid slice.  With B = one-hot planes it is the vote kernel's partial bit for bit.  The partial is rounded ONCE,
// __float2ll_rn(partial * 2^32), and added to its cell with a 64-bit integer atomic from the vector lanes, in two's complement
// (negative partials are legal here); integer addition commutes, so two runs give the same bytes, V views sum into one table
// and a split of the channels over several calls gives the columns of the one call.  Zero partials are skipped.
//
// One atomic wave-instruction covers four entries x sixteen consecutive columns: four 128-byte row segments.  The four
// quadrants of a tile are NOT merged in LDS before the atomics.
#include "ogs_common.h"
#include "../../include/ogs_query.h"

namespace ogs {
namespace {

constexpr float kAlphaMin = 1.0f / 255.0f;
constexpr float kVoteScale = 4294967296.0f;          // 2^32, kVoteScale of label_votes.hip
constexpr int kWaves = kBlock / kWave;
constexpr int kFoldRows = 16;                        // entries per batch: rows of the A tile
constexpr int kFoldCols = 16;                        // columns per MFMA block: columns of the B tile
constexpr int kFoldStride = 66;                      // row stride in words: the transposed read is bank-conflict free
// columns a wave holds in registers during one walk, 16 VGPRs per kFoldCols of them (why 32).  The
// -DOGS_EXPERIMENTS builds of scripts/feature_votes_bench.py measure 16 and 64 against it.
#if defined(OGS_EXPERIMENTS) && defined(OGS_FEATURE_VOTES_DB)
constexpr int kBlockCols = OGS_FEATURE_VOTES_DB;
#else
constexpr int kBlockCols = 32;
#endif
static_assert(kBlockCols % kFoldCols == 0 && kBlockCols >= kFoldCols, "whole MFMA blocks");
constexpr int kMaxGridY = 65535;
typedef float floatx4 __attribute__((ext_vector_type(4)));
// Timing ablations (scripts/feature_votes_bench.py: where the time goes), as in label_votes.hip: the results are WRONG by
// construction, so the switches exist only in a -DOGS_EXPERIMENTS variant build; the shipped library compiles both to `false`.
#if defined(OGS_EXPERIMENTS) && defined(OGS_VOTES_WALK_ONLY)
constexpr bool kSkipFold = true;                     // the B load and the walk alone: nothing is staged, folded or added
#else
constexpr bool kSkipFold = false;
#endif
#if defined(OGS_EXPERIMENTS) && defined(OGS_VOTES_NO_ATOMICS)
constexpr bool kSkipAtomics = true;                  // walk, staging and fold; no cell is added
#else
constexpr bool kSkipAtomics = false;
#endif

struct FeatureVotesLds {
    float4 rec[kWaves][kWave * 2];                   // per wave: geometry of the 64 entries of a sub-chunk
    int32_t row[kWaves][kWave];                      // per wave: table row of each of them, -1 = not counted
    float w[kWaves][kFoldRows * kFoldStride];        // per wave: the weights of the staged entries, [entry][pixel]
};

template <int NB>
__global__ __launch_bounds__(kBlock) void feature_votes_kernel(
    const uint2* __restrict__ ranges, const uint32_t* __restrict__ qcount, const float* __restrict__ stream, int RS,
    const uint32_t* __restrict__ quad_list, int W, int H, int gx, int tiles, const uint32_t* __restrict__ tile_order, int P,
    const float* __restrict__ features, int D, const uint8_t* __restrict__ valid, const int32_t* __restrict__ rows_of, int R,
    unsigned long long* __restrict__ votes) {
    __shared__ FeatureVotesLds lds;
    const int tile = tile_order ? (int)tile_order[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)tile >= (unsigned)tiles) return;            // block-uniform; an order the pass never wrote addresses nothing
    const int cbase = (int)blockIdx.y * (NB * kFoldCols);     // first column of this walk
    const int ncols = min(NB * kFoldCols, D + 1 - cbase);     // D + 1 columns in all: the weight column is the last
    if (ncols <= 0) return;                                   // block-uniform
    const int nblk = (ncols + kFoldCols - 1) / kFoldCols;
    const int tx = tile % gx, ty = tile / gx;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qx0 = tx * kTile + (wave & 1) * 8, qy0 = ty * kTile + (wave >> 1) * 8;
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
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

    // ---- the B tile of this walk: v(p) * F[c, p] of pixel 4 j + kq and column cbase + 16 b + m, loop invariant -------------------
    const int m = lane & 15, kq = lane >> 4;                  // operand row / column, k group
    float bv[NB][16];
    {
        const size_t plane = (size_t)H * (size_t)W;
        size_t off[16];
        uint32_t counted = 0u;                                // bit j: pixel 4 j + kq is inside the image and valid
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int p = 4 * j + kq, x = qx0 + (p & 7), y = qy0 + (p >> 3);
            const bool ok = x < W && y < H;
            off[j] = ok ? (size_t)y * (size_t)W + (size_t)x : 0;
            if (ok && (!valid || valid[off[j]] != 0)) counted |= 1u << j;
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int col = cbase + b * kFoldCols + m;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                float v = 0.f;
                if ((counted >> j) & 1u) {
                    if (col < D) v = features[(size_t)col * plane + off[j]];
                    else if (col == D) v = 1.f;               // the weight column
                }
                bv[b][j] = v;
            }
        }
    }

    int cnt = 0;                                              // wave-uniform: entries staged
    int32_t rowv = -1;                                        // lane e: table row of staged entry e
    const int64_t pitch = (int64_t)D + 1;

    auto flush = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        float a[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) a[j] = m < cnt ? wbuf[m * kFoldStride + 4 * j + kq] : 0.f;
        int32_t rowr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) rowr[r] = __shfl(rowv, 4 * kq + r, kWave);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b >= nblk) break;                             // wave-uniform
            const int col = cbase + b * kFoldCols + m;
            floatx4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = d0;
#pragma unroll
            for (int j = 0; j < 16; j += 2) {
                d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], bv[b][j], d0, 0, 0, 0);
                d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j + 1], bv[b][j + 1], d1, 0, 0, 0);
            }
            const floatx4 d = d0 + d1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = 4 * kq + r;
                const int32_t row = rowr[r];
                // every index checked where it is used: a staged row lies in [0, R), a column in [0, D]
                if (e < cnt && d[r] != 0.f && (uint32_t)row < (uint32_t)R && col >= 0 && col <= D &&
                    (!kSkipAtomics || d[r] == -1.f))
                    atomicAdd(votes + ((size_t)row * (size_t)pitch + (size_t)col),
                              (unsigned long long)__float2ll_rn(d[r] * kVoteScale));      // two's complement: the sign carries
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

size_t ogs_feature_votes_fold_columns(void) { return (size_t)kFoldCols; }
size_t ogs_feature_votes_block_columns(void) { return (size_t)kBlockCols; }

int ogs_raster_feature_votes(const OgsRasterFwdArgs* a, const OgsFeatureVotesArgs* fv, void* stream_) {
    if (!a || !fv) { set_error("feature_votes: args == NULL"); return OGS_ERR_INVALID_ARG; }
    if (a->P <= 0 || a->W <= 0 || a->H <= 0) { set_error("feature_votes: bad sizes P=%d W=%d H=%d", a->P, a->W, a->H); return OGS_ERR_INVALID_ARG; }
    if (a->C != 3 && a->C != 6 && a->C != 9 && a->C != 12) { set_error("C=%d unsupported (3, 6, 9, 12)", a->C); return OGS_ERR_UNSUPPORTED; }
    if (a->num_groups > 1) { set_error("feature_votes: grouped passes are not supported"); return OGS_ERR_UNSUPPORTED; }
    if (fv->num_channels < 1) { set_error("feature_votes: num_channels=%d", fv->num_channels); return OGS_ERR_INVALID_ARG; }
    if (fv->num_rows < 1) { set_error("feature_votes: num_rows=%d", fv->num_rows); return OGS_ERR_INVALID_ARG; }
    if (!a->image_buffer || !a->sorted_rec || !a->quad_list || !fv->features || !fv->votes) {
        set_error("feature_votes: NULL required pointer (image_buffer, sorted_rec, quad_list, features, votes)");
        return OGS_ERR_INVALID_ARG;
    }
    const int64_t walks = ((int64_t)fv->num_channels + 1 + kBlockCols - 1) / kBlockCols;      // D + 1 columns
    if (walks > kMaxGridY) {
        set_error("feature_votes: num_channels=%d needs %lld column blocks, the limit is %d", fv->num_channels, (long long)walks, kMaxGridY);
        return OGS_ERR_UNSUPPORTED;
    }
    const ImageState is = ImageState::carve(a->image_buffer, a->W, a->H, 1);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int gx = (a->W + kTile - 1) / kTile, gy = (a->H + kTile - 1) / kTile;
    const int tiles = gx * gy;
    const uint32_t* order = tile_order_of(is, tiles, a->P);        // heaviest first, as the kept pass ran
    OGS_LAUNCH_NAMED("feature_votes_kernel", feature_votes_kernel<kBlockCols / kFoldCols>, dim3((unsigned)tiles, (unsigned)walks),
               dim3(kBlock), 0, s, (const uint2*)is.ranges, (const uint32_t*)is.qcount, (const float*)a->sorted_rec, stream_vec4(a->C) * 4,
               (const uint32_t*)quad_base(a->quad_list), a->W, a->H, gx, tiles, order, a->P, fv->features, fv->num_channels,
               fv->valid, fv->rows, fv->num_rows, (unsigned long long*)fv->votes);
    OGS_LAUNCH_CHECK(a->debug, s);
    return OGS_OK;
}

}  // extern "C"
