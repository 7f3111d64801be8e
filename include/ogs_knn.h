/*
 * ogs_knn.h -- C ABI of the exact k-nearest-distance sums: for every point, the K smallest squared distances to the
 * points of its own group, reduced to three numbers.  Serves the `post_process` outlier filter of the reference's render()
 * (gaussian_renderer/__init__.py:292-309, scripts/render_by_click.py:170-189; there pytorch3d.ops.knn_points) and the
 * `distCUDA2` of simple_knn that sizes the initial scales (scene/gaussian_model.py:28-36,191).  Neither needs the
 * neighbours themselves, so none are returned and no n x n or n x K buffer exists anywhere (ogs_knn_neighbors, further
 * down, is the call that returns them).
 *
 * Rows of one group are contiguous: group g owns rows [group_begin[g], group_begin[g+1]).  group_begin must be
 * non-decreasing with values in [0, n]; offsets outside that range are clamped before anything is addressed.  Rows before
 * group_begin[0] and from group_begin[G] on belong to no group and NOTHING is written for them.
 *
 * For row i of group g with n_g rows, K = min(max(group_k[g], 0), n_g), and over ALL rows j of the group (j = i included)
 *     d2(i, j) = (dx*dx + dy*dy) + dz*dz        fp32, in this order, no contraction, dx = x_i - x_j
 *   kth[i]  = the K-th smallest d2 (0 when K = 0)
 *   sum1[i] = fp64 sum of the K smallest d2
 *   sum2[i] = fp64 sum of their squares
 * Ties at the K-th value are exact: every value below kth enters once, kth itself K - count_below times.  The result is
 * deterministic (fixed summation order).  Non-finite coordinates are undefined.
 *
 * Everything that sizes a loop is read from device memory by the kernel; the entry point does no read-back.
 * All pointers are device pointers, `stream` is a hipStream_t as void*.  Returns 0 or a negative OGS_ERR_* code.
 */
#ifndef OGS_KNN_H
#define OGS_KNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* points staged in LDS per round of the walk over a group (tests sit on both sides of it) */
size_t ogs_knn_tile_points(void);

/* points [n, 3]; group_begin [G + 1]; group_k [G]; kth [n] (may be NULL), sum1 [n], sum2 [n].
 * n <= INT32_MAX - ogs_knn_tile_points(). */
int ogs_knn_group_ksum(int64_t n, const float* points, int32_t G, const int32_t* group_begin, const int32_t* group_k,
                       float* kth, double* sum1, double* sum2, void* stream);

/*
 * The K nearest neighbours THEMSELVES, one group of all rows, at scene scale (sort once by Morton key, search in boxes).
 * For row i take every j (j = i left out when exclude_self), order by the pair (d2(i, j), j) ascending -- d2 as above, ties on
 * the distance go to the smaller index -- and store the first K: idx [n, K] int32, d2 [n, K] fp32, in the caller's row order.
 * Slots past the end of the list (n or n - 1 < K) hold idx = -1, d2 = +inf.  The result is unique, so every run gives the same
 * bytes.  1 <= K <= ogs_knn_max_k(), n * K < 2^31.  Non-finite coordinates give undefined values, never a wild address.
 * tmp: ogs_knn_neighbors_tmp_bytes(n) bytes of device scratch.
 */
size_t ogs_knn_box_points(void);                 /* points per search box (tests sit on both sides of it) */
size_t ogs_knn_max_k(void);
size_t ogs_knn_neighbors_tmp_bytes(int64_t n);
int ogs_knn_neighbors(int64_t n, const float* points, int32_t K, int32_t exclude_self, int32_t* idx, float* d2, void* tmp,
                      size_t tmp_bytes, void* stream);

/*
 * The K nearest neighbours BETWEEN TWO point sets (csrc/knn_query.hip): an index of the n REFERENCE rows, built once, and any
 * number of queries against it.  For query row q take every reference row j in [0, n), order by the pair (d2(q, j), j)
 * ascending -- d2 as above with dx = x_q - x_j, ties on the distance go to the smaller reference row -- and store the first K:
 * idx [m, K] int32 (reference rows in the caller's reference order), d2 [m, K] fp32, in the caller's query order.  Slots past the
 * end of the list (n < K) hold idx = -1, d2 = +inf.  There is no exclude_self: the two sets are unrelated.  The result is unique,
 * so two calls give the same bytes, and it does not depend on where the search of a query starts.
 *
 * index: ogs_knn_index_bytes(n) opaque device bytes that ogs_knn_index_build fills and ogs_knn_query only reads: the reference
 * coordinates sorted by Morton key in boxes of ogs_knn_box_points() points (NaN-padded to whole boxes), the sorted row numbers,
 * the bounds and the first key of every box, and the bounding box that made the keys.  It is a COPY: writing to `points` after
 * the build does not change later queries.  Valid for the n it was built with, at any address it is copied to as a whole.
 * tmp: ogs_knn_index_build_tmp_bytes(n) / ogs_knn_query_tmp_bytes(n, m) bytes of device scratch, free again after the call.
 *
 * 1 <= K <= ogs_knn_max_k(), m * K < 2^31, n and m <= INT32_MAX - ogs_knn_box_points().  n == 0 fills idx / d2 with -1 / +inf
 * (index, queries and tmp are not looked at), m == 0 does nothing, a build with n == 0 does nothing; all three return 0.  Bad
 * sizes, NULL pointers and an index or tmp that is too small return OGS_ERR_INVALID_ARG.  The size queries return 0 for a size
 * that needs no buffer or is out of range.  Non-finite coordinates on either side give undefined values, never a wild address.
 * No read-back, no float atomics, no workgroup waits on another.
 */
size_t ogs_knn_index_bytes(int64_t n);
size_t ogs_knn_index_build_tmp_bytes(int64_t n);
int ogs_knn_index_build(int64_t n, const float* points, void* index, size_t index_bytes, void* tmp, size_t tmp_bytes,
                        void* stream);
size_t ogs_knn_query_tmp_bytes(int64_t n, int64_t m);
int ogs_knn_query(int64_t n, const void* index, int64_t m, const float* queries, int32_t K, int32_t* idx, float* d2, void* tmp,
                  size_t tmp_bytes, void* stream);

/*
 * Fixed-degree gather-sum: out[i, c] = the chain acc = fmaf(w[i, k], X[idx[i, k], c], acc) from +0, k ascending, over the slots
 * with 0 <= idx[i, k] < R; other slots are skipped and their w is not read as a value.  idx, w [n, K]; X [R, D] finite;
 * out [n, D], one writer per element, no atomics.  Any D >= 1.  Its adjoint is ogs_knn_aggregate_t (gradient with respect to
 * X) and ogs_knn_edge_dots (with respect to w), below.
 */
int ogs_knn_aggregate(int64_t n, int32_t K, int64_t R, int32_t D, const int32_t* idx, const float* w, const float* X, float* out,
                      void* stream);

/*
 * ---- the graph backwards (csrc/knn_graph.hip) ------------------------------------------------------------------------------------
 * Common to everything below: no float atomics, one writer per element, no read-back; n * K < 2^31, 0 <= R <= INT32_MAX,
 * D >= 1; bad sizes, NULL pointers and a tmp that is too small return OGS_ERR_INVALID_ARG.  A slot e = i * K + k is VALID when
 * 0 <= idx[e] < R.  Two identical calls give the same bytes.
 *
 * Reverse-edge lists of idx [n, K] over R rows (R != n is allowed): begin [R + 1], slots [n * K], both int32.  For r in
 * [0, R), slots[begin[r] : begin[r + 1]] holds the valid slots e with idx[e] == r, ascending; begin[0] = 0, begin[R] = the number
 * of valid slots; a row without an incoming edge has begin[r] == begin[r + 1].  slots from begin[R] on is unspecified (written or
 * not) and nothing below reads it.  The result is unique.  tmp: ogs_knn_transpose_tmp_bytes(n, K, R) bytes.
 */
size_t ogs_knn_transpose_chunk(void);            /* slots of a list that one work item sums (tests sit on both sides of it) */
size_t ogs_knn_transpose_tmp_bytes(int64_t n, int32_t K, int64_t R);
int ogs_knn_transpose(int64_t n, int32_t K, int64_t R, const int32_t* idx, int32_t* begin, int32_t* slots, void* tmp,
                      size_t tmp_bytes, void* stream);

/*
 * Transposed gather-sum: out[r, c] = sum over the list of r of w[e] * G[e / K, c].  G [n, D], w [n, K], out [R, D]; a row with
 * an empty list gets +0.  Summation order, a function of (begin, K, D) alone -- C = ogs_knn_transpose_chunk(), m = the list's
 * length:
 *   m <= C   one chain acc = fmaf(w[e], G[e / K, c], acc) from +0 over the list in its order;
 *   m >  C   the list is cut into chunks of C slots (the last one shorter); every chunk is such a chain from +0, computed by a
 *            work item of its own, and the partials are added left to right in chunk order: ((p0 + p1) + p2) + ...
 * The four-columns-per-thread form (D % 4 == 0, G and out 16-byte aligned) and the one-column form give the same bytes.
 * begin values are clamped to [0, n * K], a pair with begin[r + 1] < begin[r] is an empty list and a slot outside [0, n * K) is
 * skipped, so no content of begin / slots makes a wild address.  The weight of an invalid slot is never read.
 * tmp: ogs_knn_aggregate_t_tmp_bytes(n, K, R, D) bytes (the work list of the split rows and their partials).
 */
size_t ogs_knn_aggregate_t_tmp_bytes(int64_t n, int32_t K, int64_t R, int32_t D);
int ogs_knn_aggregate_t(int64_t n, int32_t K, int64_t R, int32_t D, const int32_t* begin, const int32_t* slots, const float* w,
                        const float* G, float* out, void* tmp, size_t tmp_bytes, void* stream);

/*
 * Edge dots: gw[i, k] = sum_c G[i, c] * X[idx[i, k], c] on the valid slots, exactly 0 on the others.  G [n, D], X [R, D],
 * gw [n, K].  Reduction order, a function of D alone: L = the smallest power of two with 8 L >= D, at most 64; lane l of L sums the
 * columns l, l + L, ... as one chain acc = fmaf(g, x, acc) from +0; the L partials fold pairwise with the lane masks L / 2,
 * L / 4, ..., 1 (at every step the partial of lane a takes the one of lane a ^ mask).
 */
int ogs_knn_edge_dots(int64_t n, int32_t K, int64_t R, int32_t D, const int32_t* idx, const float* G, const float* X, float* gw,
                      void* stream);

/*
 * Neighbour smoothness of F [n, D] over a square graph (R = n): E = sum_i sum_k w[i, k] * |F_i - F_idx[i, k]|^2 over the valid
 * slots, differences first (coincident rows give exactly 0).
 * fwd: energy [n] fp32, energy[i] = the chain acc = fmaf(w[i, k], d2(i, k), acc) from +0, k ascending over the valid slots, with
 *      d2 = sum_c (F[i, c] - F[j, c])^2 reduced as the edge dots are (fmaf(d, d, acc) per lane, then the fold); total [2] fp64:
 *      total[0] = the sum of energy[] (two stages, both in a fixed order), total[1] = the number of valid slots.  No [n, K, D]
 *      buffer.  tmp: ogs_knn_smoothness_fwd_tmp_bytes(n) bytes.
 * bwd: gF [n, D] = 2 * scale * (sum_k w[i, k] * (F_i - F_j) + sum over the list of i of w[e] * (F_i - F_{e / K})) with `scale` a
 *      DEVICE fp32 scalar (the upstream gradient times the normalisation); begin / slots are the reverse lists of idx with R = n.
 *      Per element: the out-edge chain fmaf(w[i, k], F[i, c] - F[j, c], acc) from +0, k ascending; then the list, continued on
 *      the same accumulator when it has at most C slots, and otherwise as chunk partials from +0 that are added to it in chunk
 *      order (the split of ogs_knn_aggregate_t, the same work list); the product with 2 * scale last.  gw [n, K] (may be NULL)
 *      = scale * d2(i, k) on the valid slots, 0 on the others.  The walk over all rows and chunks is one launch; the partials of
 *      the split rows are added by a second, small one (no kernel waits on another workgroup), and gw is a launch of its own.
 *      tmp: ogs_knn_smoothness_bwd_tmp_bytes(n, K, D) bytes.
 */
size_t ogs_knn_smoothness_fwd_tmp_bytes(int64_t n);
int ogs_knn_smoothness_fwd(int64_t n, int32_t K, int32_t D, const int32_t* idx, const float* w, const float* F, float* energy,
                           double* total, void* tmp, size_t tmp_bytes, void* stream);
size_t ogs_knn_smoothness_bwd_tmp_bytes(int64_t n, int32_t K, int32_t D);
int ogs_knn_smoothness_bwd(int64_t n, int32_t K, int32_t D, const int32_t* idx, const float* w, const float* F, const int32_t* begin,
                           const int32_t* slots, const float* scale, float* gF, float* gw, void* tmp, size_t tmp_bytes,
                           void* stream);

/*
 * ---- which rows hang together (csrc/knn_components.hip) ---------------------------------------------------------------------------
 * Connected components of the graph an index table idx [n, K] spans (with d2 [n, K] as ogs_knn_neighbors writes them), under an
 * optional distance threshold and an optional same-label rule; a lock-free union-find, "hook the larger root under the smaller".
 *
 * Row i is ACTIVE when labels == NULL or labels[i] >= 0.  Slot (i, k) with j = idx[i, k] is an EDGE between i and j when all of
 *   0 <= j < n;
 *   both rows are active;
 *   labels == NULL or labels[i] == labels[j];
 *   d2 == NULL, or max_d2 == NULL, or d2[i, k] <= *max_d2 -- the fp32 compare as written: a NaN on either side gives no edge,
 *   equality gives an edge (max_d2 is a DEVICE scalar)
 * hold.  Edges are UNDIRECTED: i listing j connects them whether or not j lists i.  A self slot (j == i) is a no-op.  The
 * components are those of that graph over the active rows, numbered 0 .. C - 1 by ascending smallest member row:
 *   comp [n]   the number of the row's component, -1 for an inactive row
 *   count [1]  C
 *   sizes [n]  sizes[c] = the member count for c < C, 0 for C <= c < n
 *   first [n]  (may be NULL) first[c] = the smallest member row for c < C, -1 beyond
 * Every output element is written by every call.  The result is unique: two calls give the same bytes, and a permutation of the
 * slots within a row changes nothing.
 *
 * 1 <= K, n * K < 2^31; n == 0 writes count[0] = 0 and returns 0 (nothing else is looked at).  Bad sizes, NULL required pointers
 * (idx, comp, sizes, count, tmp) and a tmp below ogs_knn_components_tmp_bytes(n) bytes return OGS_ERR_INVALID_ARG; the size query
 * returns 0 for a size that needs no buffer or is out of range.  No read-back, no float atomics (the only read-modify-write is the
 * integer compare-and-swap of the hook; the sizes are the lengths of the components' sorted member lists), no workgroup waits on another.  No content of idx, d2 or labels makes a wild address: a slot outside [0, n) is skipped before it
 * indexes anything.  Every walk and retry loop of the union-find is bounded by a count taken from n; a thread that reaches the bound
 * sets the sticky status word (ogs_check_async_status() then returns OGS_ERR_DEVICE) and leaves its loop.
 */
size_t ogs_knn_components_tmp_bytes(int64_t n);
int ogs_knn_components(int64_t n, int32_t K, const int32_t* idx, const float* d2, const float* max_d2, const int32_t* labels,
                       int32_t* comp, int32_t* sizes, int32_t* first, int32_t* count, void* tmp, size_t tmp_bytes, void* stream);

/*
 * ---- every row within a radius (csrc/knn_radius.hip) -----------------------------------------------------------------------------
 * The walk of ogs_knn_query with a FIXED threshold: boxes of the sorted reference set are skipped by the same exact lower bound,
 * and nothing of variable length is ever stored -- memory is O(n + m) whatever the radius.  d2 as at the top of this file;
 * radius2 / eps2 is a SQUARED distance in a DEVICE fp32 scalar and the pair test is d2(q, j) <= *radius2, the fp32 compare as
 * written: equality counts, a NaN on either side counts nothing.  A NaN or negative threshold therefore selects nothing, +inf
 * every row with finite coordinates.  No read-back, no float atomics, no workgroup waits on another; two calls give the same bytes.
 *
 * ogs_knn_radius_count: count [m] int32, count[q] = the number of reference rows j in [0, n) with d2(q, j) <= *radius2, in the
 * caller's query order.  index is what ogs_knn_index_build made for the n reference rows; the queries may lie anywhere and are
 * grouped by a Morton sort of their own, as in ogs_knn_query.  Labels are given for both sets or for neither (one without the
 * other: OGS_ERR_INVALID_ARG): ref_labels [n], query_labels [m]; row j then counts only when ref_labels[j] == query_labels[q] >= 0,
 * and a query with a negative label gets 0.  Label values are compared, never used as an index.  n == 0 writes zeros (index,
 * queries, radius2 and tmp are not looked at), m == 0 does nothing.  n and m <= INT32_MAX - ogs_knn_box_points(); bad sizes, NULL
 * pointers and a tmp below ogs_knn_radius_count_tmp_bytes(n, m) bytes return OGS_ERR_INVALID_ARG.
 *
 * ogs_knn_dbscan: exact DBSCAN of one point set against itself (the sort into boxes happens inside the call, in tmp).
 *   Row i is ACTIVE when labels == NULL or labels[i] >= 0.
 *   N(i) = the active rows j with labels[j] == labels[i] (where given) and d2(i, j) <= *eps2; i itself is one of them.
 *   degree [n] (may be NULL)  |N(i)|, 0 for an inactive row
 *   core [n] uint8            degree[i] >= min_pts
 *   Clusters are the connected components of the graph on the CORE rows with an edge between two cores in each other's N.  A
 *   non-core active row with a core in N(i) is a BORDER row: it joins the cluster of the core j with the smallest pair
 *   (d2(i, j), j), that one only, and bridges nothing.  Clusters are numbered 0 .. C - 1 by ascending smallest CORE row.
 *   cluster [n]  the row's cluster, -1 for every row that is neither core nor border
 *   count [1]    C
 *   sizes [n]    sizes[c] = the members of c, borders included, for c < C; 0 beyond
 *   first [n]    (may be NULL) first[c] = the smallest core row of c for c < C; -1 beyond
 * Every output element is written by every call.  The result is unique: two calls give the same bytes, and renumbering the rows
 * gives the same partition as long as no border row has cores of two clusters at the same smallest d2.
 * min_pts >= 1, n <= INT32_MAX - ogs_knn_box_points(); n == 0 writes count[0] = 0 and returns 0 (nothing else is looked at).  Bad
 * sizes, NULL required pointers (points, eps2, cluster, core, sizes, count, tmp) and a tmp below ogs_knn_dbscan_tmp_bytes(n) bytes
 * return OGS_ERR_INVALID_ARG before anything is launched.  No content of labels makes a wild address.  The union-find is the one
 * of ogs_knn_components, bounded and reporting through the sticky status word in the same way.
 */
size_t ogs_knn_radius_count_tmp_bytes(int64_t n, int64_t m);
int ogs_knn_radius_count(int64_t n, const void* index, int64_t m, const float* queries, const float* radius2,
                         const int32_t* ref_labels, const int32_t* query_labels, int32_t* count,
                         void* tmp, size_t tmp_bytes, void* stream);
size_t ogs_knn_dbscan_tmp_bytes(int64_t n);
int ogs_knn_dbscan(int64_t n, const float* points, const float* eps2, int32_t min_pts, const int32_t* labels,
                   int32_t* cluster, uint8_t* core, int32_t* degree, int32_t* sizes, int32_t* first, int32_t* count,
                   void* tmp, size_t tmp_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OGS_KNN_H */
