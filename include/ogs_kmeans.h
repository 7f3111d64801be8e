/*
 * ogs_kmeans.h -- C ABI of the MI355X-native Lloyd k-means used by OpenGaussian's two-level codebook.
 *
 * Replaces the PyTorch ops inside /root/reference/scene/kmeans_quantize.py:
 *   Quantize_kMeans.cluster_assign  (:146-241)  cdist -> argmin -> one_hot -> mask^T @ feat per 10k chunk
 *   Quantize_kMeans.get_dist        (:38-55)    pairwise Euclidean distance
 *   Quantize_kMeans.update_centers_ (:82-87)    mask^T @ feat
 *   the gather of Quantize_kMeans.forward (:273)
 * with: one fused pairwise-L2 + argmin + segmented-reduce kernel per Lloyd iteration (features read once,
 * centres in LDS, per-workgroup LDS accumulators, fixed-order cross-workgroup reduction) and a gather.
 * The Python class opengaussian_amd.kmeans.Quantize_kMeans keeps the reference's attributes and call
 * signature and binds these functions with ctypes.
 *
 * All pointers are DEVICE pointers; feat/centers are contiguous fp32, ids are int64 (torch.long, as the
 * reference's nn_index / cls_ids).  `stream` is a hipStream_t as void*.  Returns 0 or a negative
 * OGS_ERR_* code (see ogs_raster.h); ogs_last_error() describes it.
 */
#ifndef OGS_KMEANS_H
#define OGS_KMEANS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OGS_KMEANS_MAX_DIM 16
#define OGS_KMEANS_MAX_ACC 16384   /* k * (d + 1) accumulator floats per workgroup (64 KiB of LDS) */

size_t ogs_kmeans_tmp_bytes(int64_t N, int32_t d, int32_t k);

/* `iters` Lloyd iterations followed by the final re-assignment (kmeans_quantize.py:173-240).
 *   feat      [N,d]   points
 *   centers   [k,d]   in: initial centres, out: final centres
 *   k_active  argmin considers only the first k_active rows (leaf mode: iLeafSubNum[c], :172,200);
 *             all k rows are (re)written every iteration (empty rows collapse to ~0, :211)
 *   nchunks   number of 10k chunks the reference would have looped over (root: N/10000+1, leaf: 1):
 *             reproduces its `counts += n + 1e-6` per chunk and the counts>0.1 reset (:186,213-214)
 *   ids_out   [N] int64, final argmin + id_offset
 */
int ogs_kmeans_lloyd(const float* feat, int64_t N, int32_t d, float* centers, int32_t k, int32_t k_active,
                     int32_t iters, int32_t nchunks, int64_t* ids_out, int64_t id_offset, void* tmp, void* stream);

/* Sharded Lloyd (new capability, SURVEY.md section 8(e): "k-means shards by point range"): each rank holds a
 * contiguous range of the points and the (replicated) centres.  One iteration =
 *     ogs_kmeans_accumulate(my points)        -> table [k, d+1] = per-centre feature sums | point counts
 *     all-reduce(table, SUM) over the ranks      (k*(d+1) floats: 640 at k = 64, d = 9)
 *     ogs_kmeans_update(table, ...)            -> centres, with the reference's count rule (see nchunks above)
 * `tmp` as for ogs_kmeans_lloyd (ogs_kmeans_tmp_bytes(N, d, k)).  `counts_state` [k] is the reference's
 * persistent `counts` vector: set every entry to 1e-6 before the first iteration (:167) and pass it unchanged
 * afterwards; `nchunks` is computed from the GLOBAL point count. */
int ogs_kmeans_accumulate(const float* feat, int64_t N, int32_t d, const float* centers, int32_t k, int32_t k_active,
                          float* table, void* tmp, void* stream);
int ogs_kmeans_update(const float* table, int32_t k, int32_t d, int32_t nchunks, float* counts_state, float* centers,
                      void* stream);

/* ids_out[i] = argmin_j<k ||feat[i] - centers[j]||^2 (first minimum wins, as torch.argmin) + id_offset */
int ogs_kmeans_assign(const float* feat, int64_t N, int32_t d, const float* centers, int32_t k, int64_t* ids_out,
                      int64_t id_offset, void* stream);

/* out[i, 0:out_dim] = centers[ids[i], 0:out_dim]   (forward value of the straight-through estimator,
 * kmeans_quantize.py:273-275: x - x.detach() + centres == centres) */
int ogs_kmeans_gather(const float* centers, const int64_t* ids, int64_t N, int32_t vec_dim, int32_t out_dim,
                      float* out, void* stream);

/*
 * ---- wide k-means (csrc/kmeans_wide.hip) -------------------------------------------------------------------------------------------
 * Codebooks for lifted per-Gaussian feature vectors: rows X [N, D], centres C [k, D], 1 <= D <= ogs_kmeans_wide_max_dim(),
 * 1 <= k <= ogs_kmeans_wide_max_k(), N < 2^31 (N = 0: nothing is read or launched; an update then keeps every centre).
 * Device pointers, contiguous fp32, any D and any 4-byte alignment of X, C and the outputs; tmp: 16-byte aligned device
 * scratch of ogs_kmeans_wide_tmp_bytes(N, D, k) bytes, nothing in it survives a call.  Bad sizes, an unknown metric, NULL where
 * not allowed or a tmp that is too small return OGS_ERR_INVALID_ARG.  No float atomics anywhere: two identical calls give the
 * same bytes.  Nothing is read back; everything runs on `stream`.
 *
 * assign   ids[i] = arg-max over c of  x_i . c + b_c,   b_c = -|c|^2 / 2 (L2: the nearest centre) or 0 (COSINE: C must hold
 *          unit rows; the row's own norm does not change the arg-max).  The products run on the matrix pipe as three-term bf16
 *          splits that carry both operands' 24-bit significands (six partial products per term, fp32 accumulate); for L2 both
 *          sides are first shifted by the centroid of a fixed sample of the rows.  A score is within (8 D + 64) 2^-24 of
 *          max_c (sum_j |x'_j| |c'_j| + |c'|^2 / 2) of its exact value (x', c': the shifted operands), so ids equal the exact
 *          arg-max except on near-ties of that size; exact ties go to the LOWEST centre index.  ids [N] int32.
 *          dist [N] (may be NULL) is recomputed for the winner from the inputs: L2 the fp32 sum of (x_j - c_j)^2, differences
 *          first; COSINE 1 - x . c / |x|, and 1 for a zero row.  No [N, k] buffer exists.
 * update   centre c = sum over its rows of w_i x_i / sum w_i (COSINE: then normalised), each sum in the fixed order of
 *          ogs_knn_aggregate_t over the centre's ascending row list (include/ogs_knn.h); w [N] >= 0 may be NULL (= 1).  A centre
 *          whose weights sum to 0 (COSINE: or whose sum has zero norm) keeps its previous value bit for bit.  counts [k] (may be
 *          NULL) = sum w_i.  C is read (previous) and written (new).
 * inertia  total[0] = sum_i w_i dist_i in fp64, two stages in an order that depends on N alone.
 * lloyd    iters x (assign, inertia, update), then the final assign and its inertia: inertia [iters + 1] (may be NULL),
 *          inertia[t] belongs to the assignment of iteration t; dist may be NULL; counts is what the last update wrote (not
 *          written when iters = 0).  Exactly the bytes of the same sequence made from the three calls above.
 * The sizes that shape the kernel: a workgroup scores ogs_kmeans_wide_row_tile() rows (64; 48 for D > 384, 32 for D > 512, 16 for
 * D > 768: what fits in LDS) against tiles of ogs_kmeans_wide_centre_tile() centres in steps of ogs_kmeans_wide_dim_step() dimensions, and
 * centres are packed ogs_kmeans_wide_stage() at a time.
 */
#define OGS_KMEANS_WIDE_L2 0
#define OGS_KMEANS_WIDE_COSINE 1
size_t ogs_kmeans_wide_row_tile(void);
size_t ogs_kmeans_wide_centre_tile(void);
size_t ogs_kmeans_wide_dim_step(void);
size_t ogs_kmeans_wide_stage(void);
size_t ogs_kmeans_wide_max_dim(void);
size_t ogs_kmeans_wide_max_k(void);
size_t ogs_kmeans_wide_tmp_bytes(int64_t N, int32_t D, int32_t k);      /* 0 for sizes outside the limits */
int ogs_kmeans_wide_assign(const float* X, int64_t N, int32_t D, const float* C, int32_t k, int32_t metric, int32_t* ids, float* dist,
                           void* tmp, size_t tmp_bytes, void* stream);
int ogs_kmeans_wide_update(const float* X, const float* w, int64_t N, int32_t D, const int32_t* ids, int32_t k, int32_t metric, float* C,
                           float* counts, void* tmp, size_t tmp_bytes, void* stream);
int ogs_kmeans_wide_inertia(const float* dist, const float* w, int64_t N, double* total, void* tmp, size_t tmp_bytes, void* stream);
int ogs_kmeans_wide_lloyd(const float* X, const float* w, int64_t N, int32_t D, float* C, int32_t k, int32_t metric, int32_t iters,
                          int32_t* ids, float* dist, float* counts, double* inertia, void* tmp, size_t tmp_bytes, void* stream);

/*
 * ---- wide seeding (csrc/kmeans_seed.hip) ---------------------------------------------------------------------------------------------
 * Exact k-means++ (D^2) seeding of the wide k-means: k rounds, round r draws one row with probability proportional to its mass
 * (w_i in round 0, w_i times its squared distance to the nearest centre so far afterwards) and makes it centre r.  Sizes,
 * pointers, tmp (ogs_kmeans_wide_seed_tmp_bytes), errors and `stream` as in the block above; N = 0 launches and writes nothing.
 * Inputs must be finite.  Every step is fixed below, so the result is unique: tests/kmeans_seed_restatement.py restates it in NumPy
 * and every output is equal to it byte for byte.
 *
 *   w [N] >= 0, NULL = 1.   row_scale [N], NULL = 1.   C [k, D] out: the centres.   rows [k] out: the rows they are.
 *   ids [N] out (may be NULL): the nearest seeded centre.   d2 [N] out (may be NULL): the squared distance to it.
 *   stats [4] int64 out (may be NULL): [0] centres seeded, [1] (row, round) pairs whose distance was evaluated in the rounds
 *   r >= 1, [2] pairs skipped by the bound, [1] + [2] = N (stats[0] - 1); [3] = 0.
 *
 * Points    y_ij = fl32(row_scale_i * x_ij).  L2 passes NULL; cosine passes 1 / |x_i|: D^2 sampling on the unit sphere, mass
 *           proportional to 1 - cos.  No square root and no division happens inside.
 * Distance  dist(a, b) in fp32, no FMA: t_j = fl32(fl32(a_j - b_j)^2); accumulator q (0 <= q < 256) sums the t_j with
 *           j mod 256 = q in ascending j; then s[q] = s[2 q] + s[2 q + 1], eight times, 256 values down to one.  The same order for
 *           every D and every alignment (absent terms are exact zeros).
 * Draw      rand64(seed, r) is splitmix64: z = seed + (r + 1) 0x9E3779B97F4A7C15; z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;
 *           z = (z ^ z >> 27) 0x94D049BB133111EB; z ^= z >> 31 (mod 2^64).  Masses are integers q_i < 2^31, T = their sum (exact in
 *           int64), t = (rand64 * T) >> 64, the pick is the smallest i whose inclusive prefix sum exceeds t: a row of mass 0 is never
 *           picked.
 * Round 0   q_i = floor(ldexp(w_i, 31 - E0)), E0 = the frexp exponent of max w.  C[0] = y_pick; d2_i = dist(y_i, C[0]), ids_i = 0.
 * Round r   q_i = floor(ldexp(fl32(w_i * d2_i), 31 - E)), E = the frexp exponent of max_i fl32(w_i * d2_i) after round 0, kept for
 *           all rounds (masses only fall).  C[r] = y_pick.  A row changes only when dist(y_i, C[r]) < d2_i, strictly: then d2_i is
 *           that distance and ids_i = r; ties stay with the earlier centre.
 * No mass   T = 0 before round r (fewer distinct weighted points than k): the call ends there, rows[r ..] = -1, C[r ..] is not
 *           touched, stats[0] = r.  With stats[0] = 0 (no weight at all) ids and d2 are not written either.
 * Pruning   prune != 0 skips row i in round r, unread, when with d = d2_i and b = dist(C[r], C[ids_i])
 *               d == 0   or   ( d >= 2^-100  and  fl32(b (1 - 2^-10)) >= fl32(fl32(4 d) (1 + 2^-10)) ).
 *           Proof that dist(y_i, C[r]) >= d then, so the row would not have changed.  d == 0: a distance is never negative.
 *           Otherwise write a, b', e for the exact squared distances y_i-C[ids_i], C[r]-C[ids_i], y_i-C[r]; a computed distance is
 *           within a factor 1 +- g, g = (D + 4) 2^-24 <= 2^-13, of the exact one (underflow adds at most D 2^-150, nothing beside
 *           2^-100).  (1) The rule gives b >= 4 d (1 + 2^-10), hence b' / a >= 4 (1 + 2^-10) (1 - g) / (1 + g) >= 4 (1 + 2^-11).
 *           (2) Triangle inequality: sqrt(e) >= sqrt(b') - sqrt(a) >= (2 sqrt(1 + 2^-11) - 1) sqrt(a), so e >= (1 + 2^-11) a.
 *           (3) dist(y_i, C[r]) >= e (1 - g) >= (1 + 2^-11) (1 - g) d / (1 + g) >= d.
 *           Every output has the same bytes with prune = 0 and prune = 1; only stats[1] and stats[2] differ.
 * No float atomics, no waits between workgroups, one writer per element; nothing is read back, so all k rounds are launched and the
 * rounds after the mass ran out return at once.  A workgroup of the row pass owns ogs_kmeans_wide_seed_rows() rows (256).
 */
size_t ogs_kmeans_wide_seed_rows(void);
size_t ogs_kmeans_wide_seed_tmp_bytes(int64_t N, int32_t D, int32_t k);    /* 0 for sizes outside the limits */
int ogs_kmeans_wide_seed(const float* X, const float* w, const float* row_scale, int64_t N, int32_t D, int32_t k, uint64_t seed,
                         int32_t prune, float* C, int32_t* rows, int32_t* ids, float* d2, int64_t* stats, void* tmp, size_t tmp_bytes,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OGS_KMEANS_H */
