// Pixel labels lifted to Gaussians in one walk of a finished pass (include/ogs_query.h: ogs_raster_label_votes).
//
// The transpose of label_map.hip: there every Gaussian carries a label and every pixel gets the label it shows; here every pixel
// carries a label and every Gaussian (or the row it is mapped to) gets, per label, the blend weight w_i(p) = alpha_i * T_i it puts
// on the pixels of that label, seen through the occlusion of the whole pass:
//     votes[row(g), l] += sum over the pixels p with lab(p) = l of w_{entry of g}(p)            int64, quantum 2^-32
// One workgroup per tile, wave = 8x8 quadrant, lane = pixel, the quadrant's stream 64 entries at a time with the records parked
// in LDS and broadcast, T / done / the stop rule per lane: KeptQuad::walk of kept_walk.h, the walk of label_map_kernel (this
// file is compiled with -ffp-contract=off).
//
// What is new is the per-entry reduction over the wave's 64 pixels, grouped by the pixel's label.  The labels of the 64 pixels
// are known before the walk: the wave builds its local dictionary once (first occurrence in lane order; K <= 64 distinct
// values, typically 1-3) and every pixel keeps its local index.  Entries that put weight on the quadrant and map to a counted
// row are staged sixteen at a time and folded on the matrix pipe (VoteFold of kept_walk.h, shared with feature_votes.hip) as
//     D[16 entries, 16 local labels] = Wt[16, 64 pixels] x OneHot[64, 16]          v_mfma_f32_16x16x4_f32, exact fp32
// (the fold of the features-only backward, RankOneFold in blend_bwd.hip, with the one-hot of the pixel's local index in place
// of the upstream gradient).  A quadrant with more than 16 local labels takes ceil(K / 16) column blocks over the same staged
// A tile, so any quadrant is done in ONE walk.
//
// A partial -- one entry, one quadrant, one label -- is therefore the fp32 value
//     (chain over even j of its pixels 4 j + k, k = 0..3) + (chain over odd j), every chain an fma(w, 1, acc) from +0 in pixel
//     order, the pixels of other labels entering as fma(w, 0, acc) = acc
// a function of the weights of that label's pixels and of their lane positions only: not of the label's value, of its local
// index, of its column block or of the other labels of the quadrant.  It is rounded once and added with an integer atomic
// (VoteFold::add), so two runs give the same bytes and V views sum into one table.
//
// The four quadrants of a tile are NOT merged in LDS before the atomics: a cell is (row, label), four quadrants of a tile share
// a cell only where they share a label, and DESIGN section 3b measured such merges slower than the atomics they save.
#include "kept_walk.h"
#include "../../include/ogs_query.h"

namespace ogs {
namespace {

// Timing ablations (scripts/label_votes_bench.py: where the time goes).  The results are WRONG by construction, so the switches
// exist only in a -DOGS_EXPERIMENTS variant build; the shipped library compiles both to `false`.  Each gates its step on a
// value that never occurs (a weight or a partial of -1), so the compiler keeps everything in front of the step.
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
    float4 rec[kWaves][kWave * 2];                   // per wave: the 64 parked entries of a sub-chunk (KeptQuad::walk)
    float w[kWaves][kFoldWords];                     // per wave: the weights of the staged entries (VoteFold)
    int32_t dict[kWaves][kWave];                     // per wave: label of each local index
    int32_t lidx[kWaves][kWave];                     // per wave: local index of each pixel, -1 outside the image
};

__global__ __launch_bounds__(kBlock) void label_votes_kernel(
    const uint2* __restrict__ ranges, const uint32_t* __restrict__ qcount, const float* __restrict__ stream, int RS,
    const uint32_t* __restrict__ quad_list, int W, int H, int gx, int tiles, const uint32_t* __restrict__ tile_order, int P,
    const int32_t* __restrict__ pixel_labels, int L, const int32_t* __restrict__ rows_of, int R,
    unsigned long long* __restrict__ votes) {
    __shared__ VotesLds lds;
    KeptQuad q;
    if (!q.find_tile(tiles, tile_order)) return;              // block-uniform
    q.setup(ranges, qcount, stream, RS, quad_list, W, H, gx);
    if (q.n <= 0) return;                                     // wave-uniform; no workgroup barrier follows
    const int lane = q.lane, wave = q.wave;
    const bool inside = q.inside;
    int32_t* __restrict__ dict = lds.dict[wave];

    // ---- the quadrant's local dictionary: first occurrence in lane order --------------------------------------------------------
    int32_t lab = L;
    if (inside) {
        const int32_t l = pixel_labels[(size_t)q.py * W + q.px];
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
    VoteFold fold;
    fold.init(lds.w[wave], lane);
    int32_t li[16];                                           // local index of pixel 4 j + kq: the B tile, loop invariant
#pragma unroll
    for (int j = 0; j < 16; ++j) li[j] = lds.lidx[wave][4 * j + fold.kq];
    const int nblk = (K + kFoldCols - 1) / kFoldCols;

    auto flush = [&]() {
        float a[16];
        int32_t rowr[4];
        fold.operands(a, rowr);
        for (int cb = 0; cb < nblk; ++cb) {
            const int col = cb * kFoldCols + fold.m;
            floatx4 d = VoteFold::partials(a, [&](int j) { return li[j] == col ? 1.f : 0.f; });
            if (kSkipAtomics)
                for (int r = 0; r < 4; ++r) d[r] = d[r] == -1.f ? d[r] : 0.f;      // a zero partial is not added
            fold.add(d, rowr, col < K ? dict[col] : -1, L, R, votes);               // a dictionary label lies in [0, L]
        }
        fold.reset();
    };

    // ---- the quadrant's stream, 64 entries at a time ------------------------------------------------------------------------------
    q.walk(lds.rec[wave], TableRow{rows_of, P, R}, [&](int32_t row, float w) {
        if (row >= 0 && __ballot(w != 0.f) != 0ull && (!kSkipFold || w == -1.f))
            if (fold.stage(w, row)) flush();
    });
    if (fold.cnt > 0) flush();
}

}  // namespace
}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_label_votes_quadrant_capacity(void) { return (size_t)kWave; }
size_t ogs_label_votes_fold_columns(void) { return (size_t)kFoldCols; }

int ogs_raster_label_votes(const OgsRasterFwdArgs* a, const OgsLabelVotesArgs* lv, void* stream_) {
    KeptPass kp;
    if (const int rc = kept_pass_of("label_votes", a, lv, stream_, &kp)) return rc;
    if (lv->num_labels < 0) { set_error("label_votes: num_labels=%d", lv->num_labels); return OGS_ERR_INVALID_ARG; }
    if (lv->num_rows < 1) { set_error("label_votes: num_rows=%d", lv->num_rows); return OGS_ERR_INVALID_ARG; }
    if (!kp.pointers || !lv->pixel_labels || !lv->votes) return kept_pass_null("label_votes", "pixel_labels, votes");
    OGS_LAUNCH(label_votes_kernel, dim3((unsigned)kp.tiles), dim3(kBlock), 0, kp.s, OGS_KEPT_PASS_ARGS(kp), lv->pixel_labels,
               lv->num_labels, lv->rows, lv->num_rows, (unsigned long long*)lv->votes);
    OGS_LAUNCH_CHECK(a->debug, kp.s);
    return OGS_OK;
}

}  // extern "C"
