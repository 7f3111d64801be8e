// Per-Gaussian (or per-row) D-channel features rendered into the image of a finished pass in one call (include/ogs_query.h:
// ogs_raster_feature_map).
//
// The transpose of feature_votes.hip: there a feature IMAGE goes to a table, here a TABLE X [R, D] goes to the image,
//     out[c, p] = sum over the entries e of p's tile, in depth order, of w_e(p) * X[row(g_e), c]          c < D
// over the same walk with the same weights: one workgroup per (tile, block of DB = 16 NB columns), wave = 8x8 quadrant, lane =
// pixel, the quadrant's stream 64 entries at a time with the records and rows parked in LDS and broadcast, T / done / the stop
// rule per lane -- KeptQuad::walk of kept_walk.h, the walk of feature_votes_kernel (w = alpha * T with T from before the
// update; this file is compiled with -ffp-contract=off).
//
// The fold is transposed too.  Entries that put weight on the quadrant and map to a counted row are staged sixteen at a time:
// one ds_write of the 64 weights, and a gather of the row's DB feature values (contiguous: 256 bytes at 64 columns) that
// is issued when the entry is staged and parked in LDS when the NEXT entry is staged (or at the fold), so that its latency hides
// behind the walk of the entries in between.  Then
//     Out[64 pixels, DB] += W[64 pixels, 16 entries] x X[16 entries, DB]                          v_mfma_f32_16x16x4_f32, exact fp32
// M = 16 pixels (four M-blocks cover the quadrant), K = 4 entries (four k-steps per batch), N = 16 columns: a batch takes
// 16 * DB / 16 MFMAs over 4 * DB / 16 independent accumulators that persist over the whole walk and are stored
// once after it.  The instruction is bit for bit an fmaf chain over k, k runs in depth order and the accumulator is passed whole
// from batch to batch, so per pixel and column the result is
//     acc = fmaf(w_e(p), X[row(g_e), c], acc)   from +0, over the staged entries in depth order
// An entry without weight on the pixel contributes fmaf(0, x, acc) = acc (x finite), an entry that is not staged nothing: the
// forward blend's own chain with a zero background, whichever block, walk or call the column is in.  No atomics, every output
// element has one writer: two calls give the same bytes.
//
// Output: in the C/D layout lane (j = lane & 15, kq = lane >> 4) holds pixels 16 mb + 4 kq + r of column j, i.e. four consecutive
// x of one image row.  Planar [D, H, W]: one 16-byte store per (M-block, column block) where W, H * W and the base allow it, else
// four 4-byte stores; channels-last [H, W, D]: 64 contiguous bytes per 16 lanes.  Pixels outside the image and columns >= D are
// not written; inside the image every column is, also by a quadrant without entries (zeros).
#include "kept_walk.h"
#include "../../include/ogs_query.h"

namespace ogs {
namespace {

// The transposed fold has no second user and stays here: kFoldRows entries per batch are its K (four k-steps), kFoldCols
// columns per MFMA block its N.
// columns a wave accumulates during one walk, 16 accumulator registers per kFoldCols of them.  Wider blocks divide the number of
// walks and cost registers and LDS, i.e. waves per SIMD: 64 is the widest that keeps four (DESIGN section 6m has the table: it
// ties with 32 for a single walk, wins from D = 33 on, and 128 loses everywhere).  The -DOGS_EXPERIMENTS builds of
// scripts/feature_map_bench.py measure the others against it.
#if defined(OGS_EXPERIMENTS) && defined(OGS_FEATURE_MAP_DB)
constexpr int kBlockCols = OGS_FEATURE_MAP_DB;
#else
constexpr int kBlockCols = 64;
#endif
static_assert(kBlockCols % 32 == 0 && kBlockCols >= 32, "whole MFMA blocks, and staged feature rows the k groups read without bank conflicts");
constexpr int kMaxGridY = 65535;
// Timing ablations (scripts/feature_map_bench.py: where the time goes), as in feature_votes.hip: the results are WRONG by
// construction, so the switches exist only in a -DOGS_EXPERIMENTS variant build; the shipped library compiles both to `false`.
#if defined(OGS_EXPERIMENTS) && defined(OGS_FMAP_WALK_ONLY)
constexpr bool kSkipFold = true;                     // the walk alone: nothing is staged, gathered or folded; zeros are stored
#else
constexpr bool kSkipFold = false;
#endif
#if defined(OGS_EXPERIMENTS) && defined(OGS_FMAP_NO_STORE)
constexpr bool kSkipStore = true;                    // walk, gather and fold; nothing is stored
#else
constexpr bool kSkipStore = false;
#endif

template <int NB>
struct FeatureMapLds {
    // words per staged feature row and the XOR its columns are stored under: the four k groups of a B operand read four different
    // bank quarters either way -- 64 columns and more swizzled like the weights, 32 columns through a padded stride
    static constexpr int kXStride = NB * kFoldCols >= kWave ? NB * kFoldCols : NB * kFoldCols + 16;
    static constexpr int kXSwizzle = NB * kFoldCols >= kWave ? 16 : 0;

    float4 rec[kWaves][kWave * 2];                   // per wave: the 64 parked entries of a sub-chunk (KeptQuad::walk)
    float w[kWaves][kFoldRows * kWave];              // per wave: the weights of the staged entries, [entry][pixel ^ 16 (entry & 3)]
    float x[kWaves][kFoldRows * kXStride];           // per wave: the feature rows of the staged entries, [entry][column of the walk]
};

// up to 64 columns fit four waves per SIMD: 128 registers at most, 40 KiB of LDS
template <int NB>
__global__ __launch_bounds__(kBlock, NB <= 4 ? 4 : 1) void feature_map_kernel(
    const uint2* __restrict__ ranges, const uint32_t* __restrict__ qcount, const float* __restrict__ stream, int RS,
    const uint32_t* __restrict__ quad_list, int W, int H, int gx, int tiles, const uint32_t* __restrict__ tile_order, int P,
    const float* __restrict__ features, int D, const int32_t* __restrict__ rows_of, int R, int channels_last, int vec_ok,
    float* __restrict__ out_map, float* __restrict__ out_alpha) {
    constexpr int kXStride = FeatureMapLds<NB>::kXStride, kXSwizzle = FeatureMapLds<NB>::kXSwizzle;
    constexpr int kGather = (NB * kFoldCols + kWave - 1) / kWave;      // feature values a lane gathers per staged entry
    __shared__ FeatureMapLds<NB> lds;
    KeptQuad q;
    if (!q.find_tile(tiles, tile_order)) return;              // block-uniform
    const int cbase = (int)blockIdx.y * (NB * kFoldCols);     // first column of this walk
    const int ncols = min(NB * kFoldCols, D - cbase);
    if (ncols <= 0) return;                                   // block-uniform
    const int nblk = (ncols + kFoldCols - 1) / kFoldCols;
    q.setup(ranges, qcount, stream, RS, quad_list, W, H, gx);
    const int lane = q.lane, wave = q.wave, qx0 = q.qx0, qy0 = q.qy0;      // q.n <= 0 is no exit: the quadrant owes zeros and alpha

    float* __restrict__ wbuf = lds.w[wave];
    float* __restrict__ xbuf = lds.x[wave];

    const int m = lane & 15, kq = lane >> 4;                  // operand row / column, k group
    floatx4 acc[4][NB];                                       // [M-block][column block]: pixels 16 mb + 4 kq + r, column 16 b + m
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[mb][b] = floatx4{0.f, 0.f, 0.f, 0.f};

    int cnt = 0;                                              // wave-uniform: entries staged
    int pend = -1;                                            // wave-uniform: staged entry whose gathered row is still in xg
    float xg[kGather];

    // the feature row of a staged entry: columns lane + 64 i of the walk, zero beyond D
    auto gather = [&](int32_t row) {
#pragma unroll
        for (int i = 0; i < kGather; ++i) {
            const int c = lane + kWave * i;
            float v = 0.f;
            // every index checked where it is used: a staged row lies in [0, R), a column in [0, D)
            if (c < ncols && (uint32_t)row < (uint32_t)R && cbase + c < D) v = features[(size_t)row * (size_t)D + (size_t)(cbase + c)];
            xg[i] = v;
        }
    };
    auto park = [&]() {
        if (pend < 0) return;                                 // wave-uniform
#pragma unroll
        for (int i = 0; i < kGather; ++i) {
            const int c = lane + kWave * i;
            if (c < NB * kFoldCols) xbuf[pend * kXStride + (c ^ (kXSwizzle * (pend & 3)))] = xg[i];
        }
        pend = -1;
    };

    auto fold = [&]() {
        park();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (4 * ks >= cnt) break;                         // wave-uniform: k-steps without a staged entry add nothing
            const int e = 4 * ks + kq;
            const bool live = e < cnt;                        // beyond the batch: 0 x 0, never what the staging held before
            float a[4], bx[NB];
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                const float v = wbuf[e * kWave + ((16 * mb + m) ^ (16 * kq))];
                a[mb] = live ? v : 0.f;
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const float v = xbuf[e * kXStride + ((16 * b + m) ^ (kXSwizzle * kq))];
                bx[b] = live ? v : 0.f;
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if (b >= nblk) break;                         // wave-uniform
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) acc[mb][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mb], bx[b], acc[mb][b], 0, 0, 0);
            }
        }
        cnt = 0;
        __builtin_amdgcn_wave_barrier();                      // the staging may be rewritten
    };

    // ---- the quadrant's stream, 64 entries at a time ------------------------------------------------------------------------------
    float wacc = 0.f;
    q.walk(lds.rec[wave], TableRow{rows_of, P, R}, [&](int32_t row, float w) {
        wacc += w;
        if (row >= 0 && __ballot(w != 0.f) != 0ull && (!kSkipFold || w == -1.f)) {
            park();                                                          // the previous entry's row: its load has had the walk since
            wbuf[cnt * kWave + (lane ^ (16 * (cnt & 3)))] = w;
            gather(row);
            pend = cnt;
            if (++cnt == kFoldRows) fold();
        }
    });
    if (cnt > 0) fold();

    // ---- the outputs: every in-image pixel of the quadrant, every column of this walk ------------------------------------------------
    if (out_alpha && blockIdx.y == 0 && q.inside) out_alpha[(size_t)q.py * (size_t)W + (size_t)q.px] = wacc;
    const size_t plane = (size_t)H * (size_t)W;
    const int x0 = qx0 + 4 * (kq & 1);                        // the lane's four pixels: x0 .. x0 + 3 of row qy0 + 2 mb + (kq >> 1)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b >= nblk) break;                                 // wave-uniform
        const int col = cbase + b * kFoldCols + m;
        if (col < 0 || col >= D) continue;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            const int y = qy0 + 2 * mb + (kq >> 1);
            if (y >= H) continue;
            const floatx4 d = acc[mb][b];
            if (kSkipStore && d[0] != -1.2345e30f) continue;      // the ablation keeps the fold alive and stores nothing
            if (channels_last) {
                float* __restrict__ o = out_map + (((size_t)y * (size_t)W + (size_t)x0) * (size_t)D + (size_t)col);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (x0 + r < W) o[(size_t)r * (size_t)D] = d[r];
            } else {
                float* __restrict__ o = out_map + ((size_t)col * plane + (size_t)y * (size_t)W + (size_t)x0);
                if (vec_ok) {                                 // W % 4 == 0: the four pixels are inside together; 16-byte aligned
                    if (x0 < W) *reinterpret_cast<floatx4*>(o) = d;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (x0 + r < W) o[r] = d[r];
                }
            }
        }
    }
}

}  // namespace
}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_feature_map_fold_columns(void) { return (size_t)kFoldCols; }
size_t ogs_feature_map_block_columns(void) { return (size_t)kBlockCols; }

int ogs_raster_feature_map(const OgsRasterFwdArgs* a, const OgsFeatureMapArgs* fm, void* stream_) {
    KeptPass kp;
    if (const int rc = kept_pass_of("feature_map", a, fm, stream_, &kp)) return rc;
    if (fm->num_channels < 1) { set_error("feature_map: num_channels=%d", fm->num_channels); return OGS_ERR_INVALID_ARG; }
    if (fm->num_rows < 1) { set_error("feature_map: num_rows=%d", fm->num_rows); return OGS_ERR_INVALID_ARG; }
    if (!kp.pointers || !fm->features || !fm->out_map) return kept_pass_null("feature_map", "features, out_map");
    const int64_t walks = ((int64_t)fm->num_channels + kBlockCols - 1) / kBlockCols;
    if (walks > kMaxGridY) {
        set_error("feature_map: num_channels=%d needs %lld column blocks, the limit is %d", fm->num_channels, (long long)walks, kMaxGridY);
        return OGS_ERR_UNSUPPORTED;
    }
    // planar 16-byte stores: every (column, row, x0 = multiple of 4) address is a multiple of 16 bytes
    const int vec_ok = !fm->channels_last && a->W % 4 == 0 && ((int64_t)a->W * a->H) % 4 == 0 && ((uintptr_t)fm->out_map & 15u) == 0;
    OGS_LAUNCH_NAMED("feature_map_kernel", feature_map_kernel<kBlockCols / kFoldCols>, dim3((unsigned)kp.tiles, (unsigned)walks),
                     dim3(kBlock), 0, kp.s, OGS_KEPT_PASS_ARGS(kp), fm->features, fm->num_channels, fm->rows, fm->num_rows,
                     fm->channels_last ? 1 : 0, vec_ok, fm->out_map, fm->out_alpha);
    OGS_LAUNCH_CHECK(a->debug, kp.s);
    return OGS_OK;
}

}  // extern "C"
