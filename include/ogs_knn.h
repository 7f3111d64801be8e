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
 * Fixed-degree gather-sum: out[i, c] = the chain acc = fmaf(w[i, k], X[idx[i, k], c], acc) from +0, k ascending, over the slots
 * with 0 <= idx[i, k] < R; other slots are skipped and their w is not read as a value.  idx, w [n, K]; X [R, D] finite;
 * out [n, D], one writer per element, no atomics.  Any D >= 1.  Forward only.
 */
int ogs_knn_aggregate(int64_t n, int32_t K, int64_t R, int32_t D, const int32_t* idx, const float* w, const float* X, float* out,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OGS_KNN_H */
