/*
 * ogs_refine.h -- C ABI of the multi-view SAM mask refinement (utils/sam_refinement_utils.py:1118-1318 of the
 * reference, MultiViewSAMMaskRefiner.refine_sam_masks) as batched footprint kernels.
 *
 * The reference renders ONE Gaussian per rasterizer call for every (Gaussian, camera) pair and post-processes the
 * full frame each time.  A single white Gaussian on black has closed form (T = 1, one constant colour), so a pair is
 * a few hundred evaluations of one conic; all pairs of a camera are independent.  These entry points process all
 * pairs of ONE camera per call.
 *
 * Geometry is not restated: `geom_buffer` is the geometry state ogs_raster_forward_geometry() left for this camera
 * (ogs_raster.h; `C` = the channel count of that pass), whose record rows hold
 *     { pxl, pyl, depth, radius | conic A, B, C, opacity | features }.
 * The footprint of Gaussian g is what a P = 1 pass of the rasterizer writes for it, bit for bit:
 *     alpha = min(0.99, opacity * exp(power)) inside the Gaussian's 16-px tile rectangle, 0 where power > 0 or
 *     alpha < 1/255;   q = (int) clamp(255 * (c * alpha), 0, 255)  with  c = SH_C0 * 1 + 0.5  (the white SH).
 * q is the uint8 pixel the reference's fix_image() produces; q_max = 0 means "not render-visible".
 *
 * `labels` is an int32 image [H*W] of DENSE label indices in [0, K) (the caller compacts ids with a sorted unique, so
 * the lowest id is the lowest index); an index outside [0, K) is never used as an address (the pixel is skipped).
 * All pointers are device pointers, `stream` is a hipStream_t as void*.  Returns 0 or a negative OGS_ERR_* code.
 */
#ifndef OGS_REFINE_H
#define OGS_REFINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* dominant[] codes of ogs_refine_footprint_labels for pairs it leaves to ogs_refine_footprint_labels_block */
#define OGS_REFINE_DEFER_LARGE (-2)    /* tile rectangle above OGS_REFINE_WAVE_MAX_PIXELS: a workgroup per pair */
#define OGS_REFINE_DEFER_TABLE (-3)    /* more distinct labels under the footprint than the per-wave table holds */
#define OGS_REFINE_NO_VOTE INT32_MIN   /* ogs_refine_vote: "no pair" in the input, "no winner" in the output */

/* per-wave label table: K <= capacity is indexed directly, larger K hashes the labels the footprint meets */
size_t ogs_refine_wave_table_capacity(void);
/* largest tile rectangle (pixels) the one-wave-per-pair kernel walks itself */
size_t ogs_refine_wave_max_pixels(void);
/* uint32 words of zeroed scratch per pair ogs_refine_footprint_labels_block needs (0 when K fits its LDS table) */
size_t ogs_refine_block_scratch_words(int32_t K);

/* Stage 0 (project_3d_points_to_image_batch, use_depth=True).  view / proj: the un-transposed 4x4 world-to-camera and
 * projection matrices, row-major.  visible[g] = 1 iff camera-space z > 0, 0 <= u < W, 0 <= v < H (u = ndc_x * W/2 + cx,
 * v = ndc_y * H/2 + cy, w clamped away from 0 at 1e-8) and
 * | |p - campos| - dist_optical_center - depth_map[int(v), int(u)] | < depth_diff_threshold. */
int ogs_refine_visibility(int32_t P, const float* means3D, const float* view, const float* proj, const float* campos,
                          int32_t W, int32_t H, float cx, float cy, const float* depth_map, float dist_optical_center,
                          float depth_diff_threshold, uint8_t* visible, void* stream);

/* One wave per pair i (Gaussian pairs[i]): integer sums of q per label over the footprint; dominant[i] = the label index
 * with the largest sum (ties: lowest index), or -1 when q_max[i] = 0, or an OGS_REFINE_DEFER_* code (q_max[i] is then
 * not written). */
int ogs_refine_footprint_labels(int32_t n_pairs, const int32_t* pairs, const void* geom_buffer, int32_t C, int32_t W,
                                int32_t H, const int32_t* labels, int32_t K, int32_t* dominant, int32_t* q_max,
                                void* stream);

/* One workgroup per pair, any rectangle, any K: same outputs, never defers.  `scratch`: n_pairs *
 * ogs_refine_block_scratch_words(K) zeroed uint32 (may be NULL when that is 0). */
int ogs_refine_footprint_labels_block(int32_t n_pairs, const int32_t* pairs, const void* geom_buffer, int32_t C,
                                      int32_t W, int32_t H, const int32_t* labels, int32_t K, uint32_t* scratch,
                                      int32_t* dominant, int32_t* q_max, void* stream);

/* dominant [N, cams] (global ids, OGS_REFINE_NO_VOTE where the pair does not exist): winner[g] = the id with most
 * votes in row g, ties to the id met first in camera order; OGS_REFINE_NO_VOTE for an empty row. */
int ogs_refine_vote(int64_t N, int32_t cams, const int32_t* dominant, int32_t* winner, void* stream);

/* Pairs of one camera whose dominant id is their Gaussian's winner (win[i] = its label index, q_max[i] > 0):
 * base[win[i]] += 1, and every footprint pixel with q > 0 and label != win[i] gets
 * acc[pixel * K + win[i]] += (q / 255) / (q_max / 255)  (fp32 atomics).  acc [H*W*K] and base [K] are accumulated into.
 * block_per_pair != 0: a workgroup per pair (large rectangles), otherwise a wave per pair. */
int ogs_refine_expand(int32_t n_pairs, const int32_t* pairs, const int32_t* win, const int32_t* q_max,
                      const void* geom_buffer, int32_t C, int32_t W, int32_t H, const int32_t* labels, int32_t K,
                      float* acc, int32_t* base, int32_t block_per_pair, void* stream);

/* Per pixel: channel k holds acc[pixel, k], plus on the pixel's own label (k = labels[pixel]) the initial 1.0 (0.0 when
 * k = void_index, the index of id -1, or -1 if absent) and base[k].  out[pixel] = index of the largest channel (ties:
 * lowest), or -1 where that maximum is below `threshold`. */
int ogs_refine_finalize(int64_t HW, int32_t K, const int32_t* labels, const float* acc, const int32_t* base,
                        int32_t void_index, float threshold, int32_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OGS_REFINE_H */
