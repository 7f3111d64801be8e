// Dense feature images lifted to Gaussians in one call over a finished pass (include/ogs_query.h: ogs_raster_feature_votes).
//
// label_votes.hip with a dense B operand: there every pixel carries ONE label and the fold's B tile is the one-hot of it; here
// every pixel carries a vector F[0..D)(p) and every Gaussian (or the row it is mapped to) gets the blend-weighted sum of it,
// together with the weight itself, seen through the occlusion of the whole pass:
//     table[row(g), c] += sum over the pixels p of v(p) * w_{entry of g}(p) * F[c, p]        c < D       int64, quantum 2^-32
//     table[row(g), D] += sum over the pixels p of v(p) * w_{entry of g}(p)
// v(p) = 1 inside the image where `valid` is NULL or non-zero, else 0.  One workgroup per (tile, block of kBlockCols columns),
// wave = 8x8 quadrant, lane = pixel, the quadrant's stream 64 entries at a time with the records parked in LDS and broadcast,
// T / done / the stop rule per lane: KeptQuad::walk of kept_walk.h, the walk of label_votes_kernel (w = alpha * T with T from
// before the update; this file is compiled with -ffp-contract=off).  `valid` does not touch the walk: an invalid pixel is
// occluded and occludes as any other, it only contributes to no column.
//
// The fold is the vote kernel's, VoteFold of kept_walk.h: entries that put weight on the quadrant and map to a counted row are
// staged sixteen at a time (one ds_write of the 64 weights each), then
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
#include "kept_walk.h"
#include "../../include/ogs_query.h"

namespace ogs {
namespace {

// columns a wave holds in registers during one walk, 16 VGPRs per kFoldCols of them (why 32).  The
// -DOGS_EXPERIMENTS builds of scripts/feature_votes_bench.py measure 16 and 64 against it.
#if defined(OGS_EXPERIMENTS) && defined(OGS_FEATURE_VOTES_DB)
constexpr int kBlockCols = OGS_FEATURE_VOTES_DB;
#else
constexpr int kBlockCols = 32;
#endif
static_assert(kBlockCols % kFoldCols == 0 && kBlockCols >= kFoldCols, "whole MFMA blocks");
constexpr int kMaxGridY = 65535;
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
    float4 rec[kWaves][kWave * 2];                   // per wave: the 64 parked entries of a sub-chunk (KeptQuad::walk)
    float w[kWaves][kFoldWords];                     // per wave: the weights of the staged entries (VoteFold)
};

template <int NB>
__global__ __launch_bounds__(kBlock) void feature_votes_kernel(
    const uint2* __restrict__ ranges, const uint32_t* __restrict__ qcount, const float* __restrict__ stream, int RS,
    const uint32_t* __restrict__ quad_list, int W, int H, int gx, int tiles, const uint32_t* __restrict__ tile_order, int P,
    const float* __restrict__ features, int D, const uint8_t* __restrict__ valid, const int32_t* __restrict__ rows_of, int R,
    unsigned long long* __restrict__ votes) {
    __shared__ FeatureVotesLds lds;
    KeptQuad q;
    if (!q.find_tile(tiles, tile_order)) return;              // block-uniform
    const int cbase = (int)blockIdx.y * (NB * kFoldCols);     // first column of this walk
    const int ncols = min(NB * kFoldCols, D + 1 - cbase);     // D + 1 columns in all: the weight column is the last
    if (ncols <= 0) return;                                   // block-uniform
    const int nblk = (ncols + kFoldCols - 1) / kFoldCols;
    q.setup(ranges, qcount, stream, RS, quad_list, W, H, gx);
    if (q.n <= 0) return;                                     // wave-uniform; no workgroup barrier follows
    const int qx0 = q.qx0, qy0 = q.qy0;
    VoteFold fold;
    fold.init(lds.w[q.wave], q.lane);

    // ---- the B tile of this walk: v(p) * F[c, p] of pixel 4 j + kq and column cbase + 16 b + m, loop invariant -------------------
    const int m = fold.m, kq = fold.kq;                       // operand row / column, k group
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

    auto flush = [&]() {
        float a[16];
        int32_t rowr[4];
        fold.operands(a, rowr);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b >= nblk) break;                             // wave-uniform
            floatx4 d = VoteFold::partials(a, [&](int j) { return bv[b][j]; });
            if (kSkipAtomics)
                for (int r = 0; r < 4; ++r) d[r] = d[r] == -1.f ? d[r] : 0.f;      // a zero partial is not added
            fold.add(d, rowr, cbase + b * kFoldCols + m, D, R, votes);              // a column lies in [0, D]
        }
        fold.reset();
    };

    // ---- the quadrant's stream, 64 entries at a time ------------------------------------------------------------------------------
    q.walk(lds.rec[q.wave], TableRow{rows_of, P, R}, [&](int32_t row, float w) {
        if (row >= 0 && __ballot(w != 0.f) != 0ull && (!kSkipFold || w == -1.f))
            if (fold.stage(w, row)) flush();
    });
    if (fold.cnt > 0) flush();
}

}  // namespace
}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_feature_votes_fold_columns(void) { return (size_t)kFoldCols; }
size_t ogs_feature_votes_block_columns(void) { return (size_t)kBlockCols; }

int ogs_raster_feature_votes(const OgsRasterFwdArgs* a, const OgsFeatureVotesArgs* fv, void* stream_) {
    KeptPass kp;
    if (const int rc = kept_pass_of("feature_votes", a, fv, stream_, &kp)) return rc;
    if (fv->num_channels < 1) { set_error("feature_votes: num_channels=%d", fv->num_channels); return OGS_ERR_INVALID_ARG; }
    if (fv->num_rows < 1) { set_error("feature_votes: num_rows=%d", fv->num_rows); return OGS_ERR_INVALID_ARG; }
    if (!kp.pointers || !fv->features || !fv->votes) return kept_pass_null("feature_votes", "features, votes");
    const int64_t walks = ((int64_t)fv->num_channels + 1 + kBlockCols - 1) / kBlockCols;      // D + 1 columns
    if (walks > kMaxGridY) {
        set_error("feature_votes: num_channels=%d needs %lld column blocks, the limit is %d", fv->num_channels, (long long)walks, kMaxGridY);
        return OGS_ERR_UNSUPPORTED;
    }
    OGS_LAUNCH_NAMED("feature_votes_kernel", feature_votes_kernel<kBlockCols / kFoldCols>, dim3((unsigned)kp.tiles, (unsigned)walks),
                     dim3(kBlock), 0, kp.s, OGS_KEPT_PASS_ARGS(kp), fv->features, fv->num_channels, fv->valid, fv->rows, fv->num_rows,
                     (unsigned long long*)fv->votes);
    OGS_LAUNCH_CHECK(a->debug, kp.s);
    return OGS_OK;
}

}  // extern "C"
