/*
 * ogs_query.h -- C ABI of the open-vocabulary query step that follows `cluster_lang.npz`: text features to leaves
 * (render_lerf_by_text.py:62,101-115), leaves to point classes and the confusion table behind mIoU / mAcc
 * (scripts/eval_scannet.py:143-144,158-163 and calculate_metrics, :55-93), and the stable multi-split that turns
 * OVERLAPPING leaf selections into group-contiguous row lists, so that all queries of a view go through one grouped
 * rasterizer pass and one ogs_knn_group_ksum launch (the reference: one render() and one kNN filter per (text, frame),
 * render_lerf_by_text.py:96-184).
 *
 * ---- similarity and selection (ogs_query_select) --------------------------------------------------------------------
 * One workgroup per query row q of `text` [Q, D].  For every leaf k < K
 *     sim[q, k] = leaf_valid[k] ? dot(text_q, leaf_k) / (max(|text_q|, 1e-12) * max(|leaf_k|, 1e-12)) : 0       fp32
 * (F.normalize on both sides, then the dot product; a zero row gives 0; one product and one quotient, so that D = 1
 * gives exactly +-1 as the normalised factors do).  leaf_valid == NULL: every leaf is valid.  The
 * summation order is fixed, so two calls give the same bits; it is not torch's, so sim differs from a matmul by rounding
 * (at most 2 * D * 2^-24 from the exact value).  The K similarities of a query stay in LDS for the ranking:
 * K <= ogs_query_max_leaves(), above that the call returns OGS_ERR_UNSUPPORTED.  D is arbitrary (16-byte loads over the
 * aligned part of every row, scalar loads for the rest).
 * With top > 0 (top <= ogs_query_max_top()) the R = min(top, K) highest similarities are ranked descending, ties to the
 * LOWER index, NaN never ranked.  selected[q, 0] = best = rank 0 (the argmax, lowest index on ties); every later rank c is
 * appended, in rank order, when
 *     (float)(c - best) < leaf_num      signed: every lower id qualifies (the reference's rule, kept as it is)   and
 *     || centers[best] - centers[c] ||_2 < max_dist        fp32 over center_dim values, rows of `centers` [>= K, center_dim]
 * selected [Q, top] int32 is padded with -1, count[q] = entries written.  top == 0: similarities only (selected, count,
 * centers may be NULL).
 *
 * ---- point classes (ogs_query_classify) -----------------------------------------------------------------------------
 * class_of_leaf[k] = argmax_t sim[t, k] over the T rows of sim [T, K], lowest t on ties (a zeroed leaf has an all-zero
 * column: class 0), then pred[p] = class_of_leaf[min(max(leaf_ind[p], 0), K - 1)] + 1.  The reference clamps at K - 1
 * only (:144); a negative id, which it would wrap, is clamped to 0 here and never addresses anything out of range.
 *
 * ---- confusion table (ogs_query_confusion) --------------------------------------------------------------------------
 * conf [C, C] int64 (cleared by the call): conf[g, r] = points with label g and prediction r, after
 *     g = ignore[p] ? 0 : gt[p]          (:131-132)          r = g == 0 ? 0 : pred[p]      (:58)
 * Each workgroup counts ogs_query_confusion_block() consecutive points in an LDS table of C * C counters and adds its
 * non-zero cells to `conf` with integer atomics: exact and deterministic.  C <= ogs_query_max_classes(), above that
 * OGS_ERR_UNSUPPORTED.  A point whose g or r lies outside [0, C) is NOT counted (never an out-of-range LDS index); the
 * Python wrapper checks the ranges before it calls.
 *
 * ---- stable multi-split (ogs_query_split_count / _scan / _scatter) ----------------------------------------------------
 * member(p, q) = bit q of leaf_groups[leaf_ind[p]]  &&  row_ok[p] (NULL: all)  &&  group_keep[q] (NULL: all), for
 * q < Q <= 64; a leaf id outside [0, K) (the k-means dummy id k1*k2, -1) is in no group.  The result is
 *     begin [Q + 1] int32, rows [begin[Q]] int64:  rows[begin[q] .. begin[q + 1]) = the p with member(p, q), ASCENDING
 * which is torch.nonzero(member[:, q]) group after group.  A point selected by several queries appears once per query.
 * Three launches, none of which waits for another workgroup (no spin, no look-back):
 *   count    workgroup b counts, per group, the members among its ogs_query_split_block() consecutive rows (row_ok
 *            applied, group_keep not) into tmp
 *   scan     ONE workgroup: exclusive prefix over (group, workgroup) of the counts of the kept groups -> tmp, begin;
 *            counts [Q] = the group totals BEFORE group_keep (what a caller decides group_keep by); may be run again with
 *            another group_keep over the same counts
 *   scatter  workgroup b re-derives its members and writes each at its group's offset + the rank a wave ballot gives
 * Every loop bound comes from the arguments, a leaf id is range-checked before it addresses leaf_groups (one outside
 * [0, K) is dropped, not clamped: it is in no group; only ogs_query_classify clamps), and the scatter writes no row
 * at or beyond `capacity`: a position past it (count and scatter called with different inputs) is dropped and reported
 * through the library's sticky status word, i.e. ogs_check_async_status() returns OGS_ERR_DEVICE.
 * Limits: Q <= 64 (OGS_ERR_UNSUPPORTED above), n * Q <= INT32_MAX (offsets are 32 bits; OGS_ERR_INVALID_ARG above).
 * tmp: ogs_query_split_tmp_bytes(n, Q) bytes, carried from count to scatter.
 *
 * ---- label map (ogs_raster_label_map) ----------------------------------------------------------------------------------
 * Pixel -> label: for every pixel of a finished pass, which of the per-Gaussian labels it shows.  `pass` names a finished
 * UNGROUPED streaming pass exactly as ogs_raster_forward_reblend takes it (P, W, H, C, debug, image_buffer, sorted_rec,
 * quad_list; everything else is ignored), in the layout the pass left or in the one ogs_raster_compact_kept leaves; the kept
 * buffers are only read.  For a pixel, the entries of its tile in depth order have the weights w_i = alpha_i * T_i the forward
 * blend adds to out_alpha -- same arithmetic, same candidate window, 0.99 cap, 1/255 skip and stop at T * (1 - alpha) < 1e-4 --
 * and W_l is the sum, in depth order, of the w_i whose Gaussian (slot 7 of the record) has labels[id] == l.  Then
 *     out_label  = the l with the largest W_l > 0, the LOWEST l on an exact tie, -1 where no labelled entry contributed
 *     out_weight = that W_l (0 where -1)          out_second = the largest W_l of any other label (0 if there is none)
 *     out_alpha  = the sum of ALL w_i, labelled or not: the pass's own alpha image, bit for bit
 * A label outside [0, num_labels) marks an unlabelled Gaussian: it occludes and never wins.  One launch whatever num_labels is,
 * nothing larger than the four [H, W] outputs is written, no atomic touches an output: two calls give the same bytes.  A tile
 * with more than ogs_label_map_tile_capacity() distinct labels walks its streams once per that many labels; the result is
 * exact for any tile and any num_labels.  Forward only.  Asynchronous.
 *
 * ---- label votes (ogs_raster_label_votes) --------------------------------------------------------------------------------
 * Pixel labels -> Gaussians, the transpose of the label map: how much blend weight every Gaussian puts on every label of a
 * label IMAGE of the view, through the occlusion of the whole pass.  `pass` is taken exactly as ogs_raster_label_map takes
 * it (ungrouped streaming pass, either layout, only read), and w_i(p) = alpha_i * T_i are the same weights with the same
 * arithmetic.  With
 *     lab(p) = pixel_labels[p] if it lies in [0, num_labels), else num_labels        (column L: the "no label" bucket)
 *     row(g) = g if rows == NULL, else rows[g]; a row outside [0, num_rows) is not counted (it still occludes)
 * the call ADDS to the table (the caller clears it; V views sum into one table)
 *     votes[row(g), l] += sum over the pixels p with lab(p) = l of w_{entry of g}(p)          int64 [R, L + 1], quantum 2^-32
 * Rounding: for one entry of one 8 x 8 quadrant and one label the fp32 sum over that label's pixels is a PARTIAL; it is a
 * function of the weights of those pixels and of their positions in the quadrant only (not of the label's value or of the
 * other labels of the quadrant) and is rounded once, llrint(partial * 2^32); everything after that is integer addition.  So
 * the table does not depend on the order of the atomics (two runs give the same bytes), is the same from both layouts,
 * votes(rows = r) equals index_add of votes(rows = NULL) over r, an injective relabelling of the pixels permutes the columns,
 * and two calls into one table give twice the table.
 * Range: a partial is below 2^6 (64 pixels of weight < 1), i.e. below 2^38 units; a cell must stay below 2^31 of summed
 * weight (2^63 units) over everything accumulated into it -- about 2000 full 1-megapixel images of weight 1 in ONE cell.
 * Cell addresses are computed in 64 bits; every index (Gaussian id < P, 0 <= row < R, label <= L) is checked on the device
 * before it is used, so no input makes the kernel write outside the table.  One launch whatever L is, any quadrant in one
 * walk: a quadrant's up to ogs_label_votes_quadrant_capacity() distinct labels are folded ogs_label_votes_fold_columns() at a
 * time over the same staged weights.  Forward only.  Asynchronous.
 *
 * ---- feature votes (ogs_raster_feature_votes) ------------------------------------------------------------------------------
 * Dense per-pixel vectors -> Gaussians: the label votes with a feature IMAGE F [D, H, W] (channel-planar fp32) in place of
 * the label image.  `pass`, w_i(p) and row(g) are those of ogs_raster_label_votes.  With v(p) = 1 inside the image where
 * valid == NULL or valid[p] != 0, else 0, the call ADDS to the table (the caller clears it; V views sum into one table)
 *     votes[row(g), c] += sum over the pixels p of v(p) * w_{entry of g}(p) * F[c, p]      c < D     int64 [R, D + 1], 2^-32
 *     votes[row(g), D] += sum over the pixels p of v(p) * w_{entry of g}(p)                          the weight column
 * so votes[r, :D] / votes[r, D] is the blend-weighted mean feature of row r.  An invalid pixel contributes to no column; it
 * is occluded and occludes as every other pixel (valid never changes a weight).
 * Rounding: a PARTIAL -- one entry, one 8 x 8 quadrant, one column -- is the fp32 value (fma chain over the pixels 4 j + k of
 * the even j) + (the same over the odd j), a function of the weights and of that column's 64 values v(p) * F[c, p] only, not
 * of the column's index; it is rounded once, llrint(partial * 2^32), and added in two's complement (a partial may be
 * negative).  Hence, as exact integer equalities: two runs and both layouts give the same bytes, rows = r equals index_add
 * of rows = NULL, two calls give twice the table, -F negates the columns < D, a permutation of the channels permutes the
 * columns, any split of the channels over several calls gives the columns of the one call, the weight column equals column 0
 * of ogs_raster_label_votes over the image (valid ? 0 : -1) with num_labels = 1, and one-hot planes F[c] = (lab == c) give
 * the columns of ogs_raster_label_votes.
 * Range (the caller's contract, nothing is read back to check it): F finite; a partial below 2^31, i.e. 64 * max|F| < 2^31;
 * a cell below 2^31 of summed magnitude.  Cell addresses are computed in 64 bits; every index (Gaussian id < P,
 * 0 <= row < R, column <= D) is checked on the device before it is used.  ONE call and one launch whatever D is: a wave
 * holds ogs_feature_votes_block_columns() columns in registers and the walk is repeated per such block along the grid's
 * second dimension (D + 1 <= 65535 * that); inside, the columns are folded ogs_feature_votes_fold_columns() at a time.
 * Forward only.  Asynchronous.
 *
 * ---- feature map (ogs_raster_feature_map) ----------------------------------------------------------------------------------
 * Gaussians -> dense per-pixel vectors, the transpose of the feature votes: a table X [R, D] (row-major fp32, one row per
 * Gaussian or per row(g): a leaf's CLIP / DINO / LSeg feature, say) rendered into the image of the view.  `pass`, w_i(p) and
 * row(g) are those of ogs_raster_feature_votes (ungrouped streaming pass, either layout, only read; R = P without rows).  For
 * every pixel p inside the image and every column c < D the call WRITES (it does not accumulate)
 *     out_map[c, p] = the chain acc = fmaf(w_i(p), X[row(g_i), c], acc) from +0 over the entries i of p's tile in depth order
 * over the entries whose row is counted; an entry that puts no weight on the pixel leaves acc as it is, a row outside
 * [0, num_rows) occludes and adds nothing.  That is the forward blend's own chain with a zero background: the planes equal those
 * of ceil(D / 12) ogs_raster_forward_reblend launches over [P, 12] slices of X[row(g)], bit for bit, whatever the split of the
 * columns over MFMA blocks, walks or calls.  channels_last = 0: out_map is [D, H, W]; 1: [H, W, D].
 *     out_alpha (optional) = the sum of ALL w_i, counted or not: the pass's own alpha image, bit for bit
 * so out_map / out_alpha is the blend-weighted mean feature where every row is counted, and (1 - out_alpha) * bg adds a
 * background.  No atomics, one writer per element: two calls give the same bytes; -X negates the map; a permutation of the
 * columns permutes the planes.  X must be finite (an entry without weight on a pixel is multiplied by 0, not skipped).
 * Output addresses are computed in 64 bits; every index (Gaussian id < P, 0 <= row < R, column < D, pixel inside the image) is
 * checked on the device where it is used.  ONE call and one launch whatever D is: a wave accumulates
 * ogs_feature_map_block_columns() columns per walk, ogs_feature_map_fold_columns() per MFMA block, and the walk is repeated per
 * such block along the grid's second dimension (D <= 65535 * that).  It is the adjoint of ogs_raster_feature_votes in X, which is
 * therefore its backward.  Forward only.  Asynchronous.
 *
 * No entry point reads anything back from the device.  All pointers are device pointers, `stream` is a hipStream_t as
 * void*.  Returns 0 or a negative OGS_ERR_* code.
 */
#ifndef OGS_QUERY_H
#define OGS_QUERY_H

#include <stddef.h>
#include <stdint.h>

#include "ogs_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t ogs_query_max_leaves(void);        /* K limit of ogs_query_select: one query's similarities in LDS */
size_t ogs_query_max_top(void);           /* top limit of ogs_query_select */
size_t ogs_query_max_classes(void);       /* C limit of ogs_query_confusion */
size_t ogs_query_confusion_block(void);   /* points per workgroup of ogs_query_confusion */
size_t ogs_query_split_block(void);       /* rows per workgroup of the split */
size_t ogs_query_split_tmp_bytes(int64_t n, int32_t Q);

/* text [Q, D], leaf [K, D], leaf_valid [K] bytes or NULL, centers [>= K, center_dim]; sim [Q, K], selected [Q, top],
 * count [Q] */
int ogs_query_select(int32_t Q, int32_t K, int32_t D, const float* text, const float* leaf, const uint8_t* leaf_valid,
                     const float* centers, int32_t center_dim, float leaf_num, float max_dist, int32_t top, float* sim,
                     int32_t* selected, int32_t* count, void* stream);

/* sim [T, K], leaf_ind [n]; class_of_leaf [K] int32, pred [n] int64 (n == 0: class_of_leaf only) */
int ogs_query_classify(int64_t n, const int64_t* leaf_ind, int32_t K, int32_t T, const float* sim, int32_t* class_of_leaf,
                       int64_t* pred, void* stream);

/* gt [n], pred [n], ignore [n] bytes or NULL; conf [C, C] */
int ogs_query_confusion(int64_t n, const int64_t* gt, const int64_t* pred, const uint8_t* ignore, int32_t C, int64_t* conf,
                        void* stream);

/* leaf_ind [n], leaf_groups [K], row_ok [n] bytes or NULL, group_keep [Q] bytes or NULL */
int ogs_query_split_count(int64_t n, const int64_t* leaf_ind, int32_t K, const uint64_t* leaf_groups, const uint8_t* row_ok,
                          int32_t Q, void* tmp, void* stream);
int ogs_query_split_scan(int64_t n, int32_t Q, const uint8_t* group_keep, void* tmp, int32_t* begin, int32_t* counts,
                         void* stream);
int ogs_query_split_scatter(int64_t n, const int64_t* leaf_ind, int32_t K, const uint64_t* leaf_groups,
                            const uint8_t* row_ok, int32_t Q, const uint8_t* group_keep, const void* tmp, int64_t* rows,
                            int64_t capacity, void* stream);

typedef struct OgsLabelMapArgs {
    const int32_t* labels;   /* [P]; a value outside [0, num_labels) = unlabelled: occludes, never wins */
    int32_t num_labels;      /* L >= 0, no upper limit other than int32 */
    int32_t* out_label;      /* [H,W]  winner, -1 where no labelled entry contributed */
    float* out_weight;       /* [H,W]  the winner's weight W_l (0 where -1) */
    float* out_second;       /* [H,W]  the runner-up label's weight (0 if there is none) */
    float* out_alpha;        /* [H,W]  sum of ALL weights of the pixel, labelled or not */
} OgsLabelMapArgs;
int ogs_raster_label_map(const OgsRasterFwdArgs* pass, const OgsLabelMapArgs* lm, void* stream);
size_t ogs_label_map_tile_capacity(void);   /* test hook: distinct labels of one tile handled per walk */

typedef struct OgsLabelVotesArgs {
    const int32_t* pixel_labels; /* [H,W]; a value outside [0, num_labels) counts in column num_labels */
    int32_t num_labels;          /* L >= 0 */
    const int32_t* rows;         /* [P] or NULL (row = Gaussian index); outside [0, num_rows): not counted */
    int32_t num_rows;            /* R >= 1 */
    int64_t* votes;              /* [R, L+1], quantum 2^-32, accumulated into */
} OgsLabelVotesArgs;
int ogs_raster_label_votes(const OgsRasterFwdArgs* pass, const OgsLabelVotesArgs* lv, void* stream);
size_t ogs_label_votes_quadrant_capacity(void);  /* test hook: distinct labels of one quadrant folded per walk */
size_t ogs_label_votes_fold_columns(void);       /* test hook: of those, the labels of one column block of the fold */

typedef struct OgsFeatureVotesArgs {
    const float* features;       /* [D,H,W] channel-planar, finite, 64 * max|F| < 2^31 */
    int32_t num_channels;        /* D >= 1 */
    const uint8_t* valid;        /* [H,W] or NULL (every pixel counts); 0 = the pixel contributes to no column */
    const int32_t* rows;         /* [P] or NULL (row = Gaussian index); outside [0, num_rows): not counted */
    int32_t num_rows;            /* R >= 1 */
    int64_t* votes;              /* [R, D+1], quantum 2^-32, accumulated into; column D = the weight */
} OgsFeatureVotesArgs;
int ogs_raster_feature_votes(const OgsRasterFwdArgs* pass, const OgsFeatureVotesArgs* fv, void* stream);
size_t ogs_feature_votes_fold_columns(void);     /* test hook: columns of one MFMA block of the fold */
size_t ogs_feature_votes_block_columns(void);    /* test hook: columns a wave holds per walk; D + 1 columns take ceil((D + 1) / this) walks */

typedef struct OgsFeatureMapArgs {
    const float* features;       /* [R, D] row-major fp32, finite */
    int32_t num_channels;        /* D >= 1 */
    const int32_t* rows;         /* [P] or NULL (row = Gaussian index, R = P); outside [0, num_rows): occludes, adds nothing */
    int32_t num_rows;            /* R >= 1 */
    int32_t channels_last;       /* 0: out_map [D,H,W] planar;  1: out_map [H,W,D] */
    float* out_map;              /* every in-image element is written by the call (not accumulated into) */
    float* out_alpha;            /* [H,W] or NULL: the sum of ALL weights of the pixel */
} OgsFeatureMapArgs;
int ogs_raster_feature_map(const OgsRasterFwdArgs* pass, const OgsFeatureMapArgs* fm, void* stream);
size_t ogs_feature_map_fold_columns(void);       /* test hook: columns of one MFMA block */
size_t ogs_feature_map_block_columns(void);      /* test hook: columns a wave accumulates per walk; D columns take ceil(D / this) walks */

#ifdef __cplusplus
}
#endif
#endif /* OGS_QUERY_H */
