// Per-pixel dominant label of a finished pass (include/ogs_query.h: ogs_raster_label_map).
//
// A kept ungrouped streaming pass (image_buffer, packed records, quadrant streams: what ogs_raster_forward_reblend walks) already
// holds everything that decides, for every pixel, which label it shows: the weights w_i = alpha_i * T_i the forward blend adds to
// out_alpha.  One workgroup per tile walks the tile's four quadrant streams again and sums the weights per label,
//     W_l = sum of w_i over the entries whose Gaussian carries label l, in depth order,
// in a dense LDS table of kLabelCap rows x 256 pixels; winner, winner's weight, runner-up weight and alpha come out of one
// launch and O(H * W) memory whatever the number of labels.
//
// Which label owns which row is decided per tile, without a hash and without anything that depends on arrival order:
//   * the workgroup scans the labels of the tile's kept records (labels[id], id = slot 7 of a record) and marks those inside a
//     WINDOW of kWindowBits consecutive label values in an LDS bitmap (ds_or: the bitmap is the same whatever the order); the
//     smallest label beyond the window comes out of the same scan (ds_min) and is where the next window starts, so empty stretches
//     of the label range cost nothing and any L works;
//   * a label's rank among the set bits (prefix popcount) is its local index: ascending in the label, so the rows of a window,
//     the sub-passes of a window and the windows themselves visit the labels in ascending order, and "largest weight, lowest label
//     on a tie" is a strict compare against the running best;
//   * a window with more than kLabelCap labels takes ceil(K / kLabelCap) sub-passes; every sub-pass walks the streams again with
//     the same arithmetic (same T, same stop, same alpha) and carries (best, second) in registers.  Exact for any tile.
// Every lane owns its pixel's column of the table (address row * 256 + pixel: consecutive lanes, consecutive banks), so the update
// is a plain LDS read-add-write; nothing is an atomic on the outputs and two runs give the same bits.
//
// The per-pixel arithmetic restates QuadWalk::consume (blend_fwd.hip) as refine.hip does: blend_power, the candidate window
// |power + h| <= h, min(0.99, opacity * __expf(power)), the 1/255 skip and the stop at T * (1 - alpha) < 1e-4, in the same
// operation order; this file is compiled with -ffp-contract=off, so the sums are the plain adds the blend makes.  The 4x4-block
// sublists of QuadWalk::step are a speed device of the blend (a skipped (entry, block) pair is one every pixel of the block skips
// anyway) and are not restated: a wave takes its quadrant's stream 64 entries at a time, lane e parks record e and its row in
// LDS, and the wave walks the 64 entries with the record broadcast from LDS.
#include "ogs_common.h"
#include "../../include/ogs_query.h"

namespace ogs {
namespace {

constexpr float kAlphaMin = 1.0f / 255.0f;
constexpr int kLabelCap = 64;                        // rows of the dense table: 64 x 256 x 4 B = 64 KiB, two workgroups per CU
constexpr int kWindowBits = 32 * kBlock;             // label values per window: one bitmap word per thread
constexpr int kWaves = kBlock / kWave;

struct LabelLds {
    float table[kLabelCap * kBlock];                 // [row][pixel]
    float4 rec[kWaves][kWave * 2];                   // per wave: geometry of the 64 entries of a sub-chunk
    int32_t row[kWaves][kWave];                      // per wave: table row of each of them, -1 = none
    uint32_t bits[kBlock];                           // labels of the window present in the tile
    uint32_t prefix[kBlock];                         // set bits in front of each word
    int32_t row_label[kLabelCap];                    // global label of each row of the current sub-pass
    uint32_t wave_tot[kWaves];
    uint32_t next;                                   // smallest label of the tile beyond the window (0xFFFFFFFF: none)
};

__global__ __launch_bounds__(kBlock) void label_map_kernel(
    const uint2* __restrict__ ranges, const uint32_t* __restrict__ qcount, const float* __restrict__ stream, int RS,
    const uint32_t* __restrict__ quad_list, int W, int H, int gx, int tiles, const uint32_t* __restrict__ tile_order, int P,
    const int32_t* __restrict__ labels, int L, int32_t* __restrict__ out_label, float* __restrict__ out_weight,
    float* __restrict__ out_second, float* __restrict__ out_alpha) {
    __shared__ LabelLds lds;
    const int tile = tile_order ? (int)tile_order[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)tile >= (unsigned)tiles) return;            // block-uniform; an order the pass never wrote addresses nothing
    const int tx = tile % gx, ty = tile / gx;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int px = tx * kTile + (wave & 1) * 8 + (lane & 7);
    const int py = ty * kTile + (wave >> 1) * 8 + (lane >> 3);
    const bool inside = px < W && py < H;
    const float fx = (float)px, fy = (float)py;

    // both layouts with one formula (blend_forward_rows_kernel): the tile owns n_tile slots at range.x, of which it packed n_kept
    const uint2 range = ranges[tile];
    const int n_tile = (int)(range.y - range.x);
    const int n = min((int)qcount[tile * 5 + wave], n_tile), n_kept = min((int)qcount[tile * 5 + 4], n_tile);
    const float* __restrict__ tb = stream + (size_t)range.x * RS;
    const uint32_t* __restrict__ qi = quad_list + ((size_t)range.x * 5 + (size_t)wave * n_tile);
    const uint32_t lim = n_kept > 0 ? (uint32_t)n_kept - 1u : 0u;

    auto label_of = [&](float id_bits) -> int32_t {
        const uint32_t id = __float_as_uint(id_bits);
        const int32_t l = id < (uint32_t)P ? labels[id] : -1;
        return (l >= 0 && l < L) ? l : -1;
    };

    // ---- phase A: which labels of [lo, lo + kWindowBits) does the tile hold, and where does the next window start -------------
    // returns the window's label count; `next` < 0: no label beyond the window
    auto scan_window = [&](int64_t lo, int64_t& next) -> int {
        __syncthreads();                                      // the previous window's bitmap is no longer read
        lds.bits[tid] = 0u;
        if (tid == 0) lds.next = 0xFFFFFFFFu;
        __syncthreads();
        const int64_t hi = lo + kWindowBits;
        for (int i = tid; i < n_kept; i += kBlock) {
            const int32_t l = label_of(tb[(size_t)i * RS + 7]);
            if (l < 0) continue;
            if ((int64_t)l >= hi) {
                atomicMin(&lds.next, (uint32_t)l);
            } else if ((int64_t)l >= lo) {
                const uint32_t rel = (uint32_t)((int64_t)l - lo);
                atomicOr(&lds.bits[rel >> 5], 1u << (rel & 31u));
            }
        }
        __syncthreads();
        const uint32_t c = (uint32_t)__popc(lds.bits[tid]);
        uint32_t inc = c;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t t = __shfl_up(inc, d, kWave);
            if (lane >= d) inc += t;
        }
        if (lane == kWave - 1) lds.wave_tot[wave] = inc;
        __syncthreads();
        uint32_t before = 0u, total = 0u;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const uint32_t t = lds.wave_tot[w];
            if (w < wave) before += t;
            total += t;
        }
        lds.prefix[tid] = before + inc - c;
        const uint32_t nx = lds.next;
        next = nx == 0xFFFFFFFFu ? (int64_t)-1 : (int64_t)nx;
        __syncthreads();
        return (int)total;
    };

    int64_t lo = -(int64_t)kWindowBits, next = -1;            // an empty window in front of label 0: finds the smallest label
    int K = scan_window(lo, next);
    if (next >= 0) {
        lo = next;
        K = scan_window(lo, next);
    }

    float best = 0.f, second = 0.f, wacc = 0.f;
    int32_t best_label = -1;
    float* __restrict__ col = lds.table + tid;                // this pixel's column
    float4* __restrict__ recs = lds.rec[wave];
    int32_t* __restrict__ rows = lds.row[wave];

    for (;;) {                                                // windows (block-uniform: K and next come from LDS)
        const int subs = max(1, (K + kLabelCap - 1) / kLabelCap);      // a tile without labels still owes its alpha: one walk
        for (int s = 0; s < subs; ++s) {
            const int r0 = s * kLabelCap, nrows = max(0, min(kLabelCap, K - r0));
            __syncthreads();                                  // row_label of the previous sub-pass is no longer read
            {
                uint32_t w = lds.bits[tid];
                int rank = (int)lds.prefix[tid] - r0;
                while (w != 0u && rank < kLabelCap) {
                    const int b = __ffs((int)w) - 1;
                    if (rank >= 0) lds.row_label[rank] = (int32_t)(lo + (int64_t)(tid * 32 + b));
                    w &= w - 1u;
                    ++rank;
                }
            }
            for (int r = 0; r < nrows; ++r) col[r * kBlock] = 0.f;
            __syncthreads();

            // ---- phase B: the quadrant's stream, 64 entries at a time ------------------------------------------------------------
            float T = 1.0f;
            bool done = !inside;
            wacc = 0.f;
            for (int c0 = 0; c0 < n && __ballot(!done) != 0ull; c0 += kWave) {
                const int cnt = min(kWave, n - c0);
                if (lane < cnt) {
                    const uint32_t ridx = min(qi[c0 + lane], lim);
                    const float4* __restrict__ rp = reinterpret_cast<const float4*>(tb + (size_t)ridx * RS);
                    const float4 g0 = rp[0], g1 = rp[1];
                    int32_t row = -1;
                    const int32_t l = label_of(g1.w);
                    if (l >= 0 && (int64_t)l >= lo && (int64_t)l < lo + kWindowBits) {
                        const uint32_t rel = (uint32_t)((int64_t)l - lo);
                        const uint32_t word = lds.bits[rel >> 5], bit = 1u << (rel & 31u);
                        const int rank = (int)lds.prefix[rel >> 5] + __popc(word & (bit - 1u)) - r0;
                        if ((word & bit) != 0u && rank >= 0 && rank < nrows) row = rank;
                    }
                    recs[lane * 2] = g0;
                    recs[lane * 2 + 1] = g1;
                    rows[lane] = row;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (int e = 0; e < cnt && __ballot(!done) != 0ull; ++e) {
                    const float4 g0 = recs[e * 2], g1 = recs[e * 2 + 1];         // x y a2 c2 | b2 h opacity id
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
                    wacc += w;
                    const int32_t row = rows[e];
                    if (row >= 0) col[row * kBlock] += w;                       // wave-uniform row, the lane's own slot
                }
                __builtin_amdgcn_wave_barrier();                                 // the staging may be rewritten
            }

            // ---- the rows of this sub-pass, ascending in the label ---------------------------------------------------------------
            for (int r = 0; r < nrows; ++r) {
                const float w = col[r * kBlock];
                if (w > best) {
                    second = best;
                    best = w;
                    best_label = lds.row_label[r];
                } else if (w > second) {
                    second = w;
                }
            }
        }
        if (next < 0) break;
        lo = next;
        K = scan_window(lo, next);
    }

    if (inside) {
        const size_t pix = (size_t)py * W + px;
        out_label[pix] = best_label;
        out_weight[pix] = best;
        out_second[pix] = second;
        out_alpha[pix] = wacc;
    }
}

}  // namespace
}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_label_map_tile_capacity(void) { return (size_t)kLabelCap; }

int ogs_raster_label_map(const OgsRasterFwdArgs* a, const OgsLabelMapArgs* lm, void* stream_) {
    if (!a || !lm) { set_error("label_map: args == NULL"); return OGS_ERR_INVALID_ARG; }
    if (a->P <= 0 || a->W <= 0 || a->H <= 0) { set_error("label_map: bad sizes P=%d W=%d H=%d", a->P, a->W, a->H); return OGS_ERR_INVALID_ARG; }
    if (a->C != 3 && a->C != 6 && a->C != 9 && a->C != 12) { set_error("C=%d unsupported (3, 6, 9, 12)", a->C); return OGS_ERR_UNSUPPORTED; }
    if (a->num_groups > 1) { set_error("label_map: grouped passes are not supported"); return OGS_ERR_UNSUPPORTED; }
    if (lm->num_labels < 0) { set_error("label_map: num_labels=%d", lm->num_labels); return OGS_ERR_INVALID_ARG; }
    if (!a->image_buffer || !a->sorted_rec || !a->quad_list || !lm->labels || !lm->out_label || !lm->out_weight || !lm->out_second ||
        !lm->out_alpha) {
        set_error("label_map: NULL required pointer (image_buffer, sorted_rec, quad_list, labels, out_*)");
        return OGS_ERR_INVALID_ARG;
    }
    const ImageState is = ImageState::carve(a->image_buffer, a->W, a->H, 1);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int gx = (a->W + kTile - 1) / kTile, gy = (a->H + kTile - 1) / kTile;
    const int tiles = gx * gy;
    const uint32_t* order = tile_order_of(is, tiles, a->P);        // heaviest first, as the kept pass ran
    OGS_LAUNCH(label_map_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, s, (const uint2*)is.ranges, (const uint32_t*)is.qcount,
               (const float*)a->sorted_rec, stream_vec4(a->C) * 4, (const uint32_t*)quad_base(a->quad_list), a->W, a->H, gx, tiles,
               order, a->P, lm->labels, lm->num_labels, lm->out_label, lm->out_weight, lm->out_second, lm->out_alpha);
    OGS_LAUNCH_CHECK(a->debug, s);
    return OGS_OK;
}

}  // extern "C"
