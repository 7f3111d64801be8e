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
// The walk itself -- quadrant set-up, the 64-entry staging with the entry's table row in the record's id slot, and the per-pixel
// chain whose sums are the plain adds the blend makes -- is KeptQuad of kept_walk.h; this file is compiled with
// -ffp-contract=off.
#include "kept_walk.h"
#include "../../include/ogs_query.h"

namespace ogs {
namespace {

constexpr int kLabelCap = 64;                        // rows of the dense table: 64 x 256 x 4 B = 64 KiB, two workgroups per CU
constexpr int kWindowBits = 32 * kBlock;             // label values per window: one bitmap word per thread

struct LabelLds {
    float table[kLabelCap * kBlock];                 // [row][pixel]
    float4 rec[kWaves][kWave * 2];                   // per wave: the 64 parked entries of a sub-chunk (KeptQuad::walk)
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
    KeptQuad q;
    if (!q.find_tile(tiles, tile_order)) return;              // block-uniform
    q.setup(ranges, qcount, stream, RS, quad_list, W, H, gx);
    const int tid = threadIdx.x, lane = q.lane, wave = q.wave, n_kept = q.n_kept;
    const float* __restrict__ tb = q.tb;

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
            wacc = 0.f;
            q.walk(
                lds.rec[wave],
                [&](float id_bits) -> int32_t {               // the label's rank in the window, where this sub-pass holds it
                    const int32_t l = label_of(id_bits);
                    if (l < 0 || (int64_t)l < lo || (int64_t)l >= lo + kWindowBits) return -1;
                    const uint32_t rel = (uint32_t)((int64_t)l - lo);
                    const uint32_t word = lds.bits[rel >> 5], bit = 1u << (rel & 31u);
                    const int rank = (int)lds.prefix[rel >> 5] + __popc(word & (bit - 1u)) - r0;
                    return ((word & bit) != 0u && rank >= 0 && rank < nrows) ? rank : -1;
                },
                [&](int32_t row, float w) {
                    wacc += w;
                    if (row >= 0) col[row * kBlock] += w;     // wave-uniform row, the lane's own slot
                });

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

    if (q.inside) {
        const size_t pix = (size_t)q.py * W + q.px;
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
    KeptPass kp;
    if (const int rc = kept_pass_of("label_map", a, lm, stream_, &kp)) return rc;
    if (lm->num_labels < 0) { set_error("label_map: num_labels=%d", lm->num_labels); return OGS_ERR_INVALID_ARG; }
    if (!kp.pointers || !lm->labels || !lm->out_label || !lm->out_weight || !lm->out_second || !lm->out_alpha)
        return kept_pass_null("label_map", "labels, out_*");
    OGS_LAUNCH(label_map_kernel, dim3((unsigned)kp.tiles), dim3(kBlock), 0, kp.s, OGS_KEPT_PASS_ARGS(kp), lm->labels, lm->num_labels,
               lm->out_label, lm->out_weight, lm->out_second, lm->out_alpha);
    OGS_LAUNCH_CHECK(a->debug, kp.s);
    return OGS_OK;
}

}  // extern "C"
