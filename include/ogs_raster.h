/*
 * ogs_raster.h -- C ABI of the MI355X-native differentiable Gaussian tile rasterizer.
 *
 * This is the drop-in boundary for the native half of the reference's rasterizer package
 * `ashawkey_diff_gaussian_rasterization` (imported at
 * /root/reference/gaussian_renderer/__init__.py:15 and utils/sam_refinement_utils.py:21; its
 * C++/CUDA source is NOT vendored, see .MISSING_LARGE_BLOBS:1).  The entry points below are what
 * that package's Python side binds as `_C.rasterize_gaussians`, `_C.rasterize_gaussians_backward`
 * and `_C.mark_visible`, restated as plain C: raw device pointers,
 * sizes and a HIP stream handle -- no torch types.  The Python facade
 * (opengaussian_amd/rasterizer.py) binds them with ctypes; INTEGRATION.md shows the stub.
 *
 * All pointers are DEVICE pointers to contiguous fp32 / int32 data unless stated otherwise.
 * `stream` is a hipStream_t passed as void* (0 = the null stream).  Every function returns
 * OGS_OK (0) or a negative OGS_ERR_* code; ogs_last_error() returns a static description.
 * Inputs are borrowed and never written.
 *
 * Forward is split in two calls because the size of the per-(Gaussian,tile) list
 * (`num_rendered`) is only known after the geometry phase:
 *
 *   ogs_raster_forward_geometry()  preprocess -> scan (P > 1024, default binning: per-workgroup sums -> offsets)   (A.1, first half of A.2)
 *        -> host learns num_rendered, allocates point_list / binning scratch
 *   ogs_raster_forward_render()    duplicate -> tile sort -> ranges -> per-tile depth sort -> blend   (A.2, A.3)
 *   (grouped passes and P <= 1024 sort the Gaussians by depth in the geometry phase instead of each tile's list)
 *
 * Replaces the single upstream call `rasterize_gaussians(bg, means3D, colors, opacity, scales,
 * rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, H, W, sh,
 * degree, campos, prefiltered, debug)` used through GaussianRasterizer.forward at
 * gaussian_renderer/__init__.py:104-112,129-163,203-225,327-345.
 */
#ifndef OGS_RASTER_H
#define OGS_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OGS_OK 0
#define OGS_ERR_INVALID_ARG (-1)
#define OGS_ERR_HIP (-2)
#define OGS_ERR_UNSUPPORTED (-3)
#define OGS_ERR_SCRATCH_TOO_SMALL (-4)
#define OGS_ERR_DEVICE (-5)    /* a kernel of an earlier launch reported a condition it could not recover from (sticky status
                                * word, ogs_check_async_status): the results since the last check are not valid */

#define OGS_TILE 16            /* BLOCK_X = BLOCK_Y = 16 */
#define OGS_MAX_CHANNELS 12    /* blended feature channels per pass: 3 (facade), 6, 9, 12 (fused) */

/* Arguments of one forward pass.  Mirrors the argument list of the reference's
 * rasterize_gaussians (see file header); `C` generalises its NUM_CHANNELS=3. */
typedef struct OgsRasterFwdArgs {
    int32_t P;               /* number of Gaussians */
    int32_t W, H;            /* image size in pixels */
    int32_t C;               /* blended channels (3 for the drop-in facade) */
    int32_t sh_degree;       /* active SH degree 0..3 (used when shs != NULL) */
    int32_t sh_coeffs;       /* M: coefficients per Gaussian stored in shs ([P,M,3]) */
    float tanfovx, tanfovy;
    float scale_modifier;
    int32_t prefiltered;     /* accepted for API parity; unused (as upstream) */
    int32_t debug;           /* !=0: synchronise + check after every kernel */
    const float* bg;             /* [C] */
    const float* means3D;        /* [P,3] */
    const float* colors_precomp; /* shs == NULL: [P,C] all blended channels.
                                    shs != NULL and C > 3 (fused pass): [P,C-3] extra channels 3..C-1 */
    const float* shs;            /* [P,M,3] or NULL; fills channels 0..2 (C == 3, or C > 3 with extra channels) */
    const float* opacities;      /* [P] */
    const float* scales;         /* [P,3] or NULL */
    const float* rotations;      /* [P,4] or NULL */
    const float* cov3D_precomp;  /* [P,6] or NULL */
    const float* viewmatrix;     /* [16] row-major W2C^T (scene/cameras.py:71) */
    const float* projmatrix;     /* [16] row-major W2C^T @ P^T (scene/cameras.py:76) */
    const float* campos;         /* [3] */
    float* out_color;            /* [C,H,W] */
    float* out_depth;            /* [1,H,W] */
    float* out_alpha;            /* [1,H,W] */
    int32_t* radii;              /* [P] */
    void* geom_buffer;           /* ogs_raster_geom_bytes(P, C): kept until backward */
    void* geom_tmp;              /* ogs_raster_geom_tmp_bytes(P): must live across both forward calls */
    void* image_buffer;          /* ogs_raster_image_bytes(W, H): kept until backward */
    uint32_t* point_list;        /* capacity [num_rendered]: sorted Gaussian ids in bits 0..30; bit 31: the (Gaussian, tile) pair
                                  * can reach a pixel of its tile (P < 2^31).  Default mode: only the reachable pairs are listed
                                  * (the tile ranges say how many); full_binning != 0: all num_rendered pairs.  Kept until
                                  * backward (render phase) */
    void* binning_tmp;           /* ogs_raster_binning_tmp_bytes(num_rendered, W, H) (render phase) */
    void* sorted_rec;            /* ogs_raster_sorted_bytes(num_rendered, C): one packed record per sorted-list entry,
                                    read by the blend kernels through the scalar path; kept until backward */
    void* quad_list;             /* ogs_raster_quad_list_bytes(num_rendered): per (tile, 8x8 quadrant) the tile-local
                                    indices of the entries that can reach the quadrant; kept until backward */
    /* Grouped pass ("batched subset rendering via a per-Gaussian group_id"): with
     * num_groups = G > 1 the pass renders G independent images in one go -- image g blends exactly the
     * Gaussians with group_ids[p] == g, i.e. what G separate calls on the boolean-indexed subsets
     * (gaussian_renderer/__init__.py:203-225,327-345) would return -- sharing one preprocess, one sort and one
     * launch sequence.  out_color is then [G,C,H,W], out_depth / out_alpha [G,1,H,W], image_buffer
     * ogs_raster_image_bytes_grouped(W, H, G); Gaussians with a group id outside [0, G) are not rendered
     * (radius 0).  num_groups <= 1 (and group_ids == NULL): the plain single-image pass. */
    const int32_t* group_ids;    /* [P] or NULL */
    int32_t num_groups;          /* 0 or 1: ungrouped */
    int32_t full_binning;        /* 0 (default): the (Gaussian, tile) pairs that cannot reach alpha >= 1/255 on any pixel of their
                                  * tile are dropped before the tile sort -- point_list, the tile ranges and what
                                  * ogs_raster_export_binning returns hold the reachable pairs only, in the reference's order
                                  * (images and gradients do not change: those pairs contribute nothing).  != 0: the reference's
                                  * full list (every tile of every footprint rectangle), the unreachable pairs flagged in bit 31
                                  * of point_list.  (Occupies what used to be tail padding: the struct size is unchanged.) */
    /* Optional (render phase): a range the forward blend zeroes on the way -- the gradient record ogs_raster_backward would
     * otherwise clear with a fill launch of its own between two kernels that cannot overlap it (128 B per Gaussian, 17 us at
     * 1 M Gaussians), written here by a kernel that is not bandwidth-bound.  NULL: nothing is cleared.  Non-NULL: 16-byte
     * aligned, bwd_clear_bytes a multiple of 16; when ogs_raster_forward_render / _deferred returns OGS_OK the range will be
     * zero in stream order, whatever the pass looks like (an empty list and the passes whose blend does not host the stores
     * clear it with a fill).  The caller then sets OgsRasterBwdArgs.bwd_tmp_is_clear.  Ignored by every other entry point. */
    void* bwd_clear;
    size_t bwd_clear_bytes;
} OgsRasterFwdArgs;

/* Arguments of the backward pass.  Mirrors upstream rasterize_gaussians_backward(bg, means3D,
 * radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
 * tan_fovx, tan_fovy, dL_dcolor, dL_ddepth, dL_dalpha, sh, degree, campos, geomBuffer, R,
 * binningBuffer, imgBuffer, alpha, debug).  Any output pointer may be NULL to skip that
 * gradient family (stages 1-2 only need dL_dcolors).  When dL_dcolors is the ONLY
 * non-NULL output (every Gaussian parameter but `_ins_feat` detached, train.py:431-436, and the caller does not
 * consume dL_dmeans2D -- it only feeds densification, train.py:594-598) the pass runs its features-only kernels:
 * no alpha-gradient recursion, no geometry partials, no per-Gaussian geometry backward. */
typedef struct OgsRasterBwdArgs {
    int32_t P, W, H, C, sh_degree, sh_coeffs;
    float tanfovx, tanfovy, scale_modifier;
    int32_t debug;
    int32_t num_rendered;
    int32_t geom_channels;       /* 0 or C: every channel feeds the geometry/opacity gradients (reference
                                    behaviour).  3 (with C > 3): only channels 0..2 + depth + alpha do; channels
                                    >= 3 just receive dL/dfeature (fused RGB + detached ins_feat pass).  Other
                                    values are rejected (the value is a compile-time constant of the kernel). */
    const float* bg;
    const float* means3D;
    const float* colors_precomp;
    const float* shs;
    const float* opacities;
    const float* scales;
    const float* rotations;
    const float* cov3D_precomp;
    const float* viewmatrix;
    const float* projmatrix;
    const float* campos;
    const int32_t* radii;        /* [P] from forward */
    const float* out_alpha;      /* [1,H,W] from forward: accepted for parity with upstream's argument list, may be NULL.
                                    Upstream starts the backward's transmittance recursion from 1 - out_alpha; here the
                                    forward keeps its exact final T per pixel in image_buffer (4 B/pixel) and the
                                    backward starts from that: 1 - alpha in fp32 is off by up to 6e-4 relative on
                                    saturated pixels, and that error would scale every gradient of the pixel. */
    const float* dL_dcolor;      /* [C,H,W] */
    const float* dL_ddepth;      /* [1,H,W] or NULL (= zeros) */
    const float* dL_dalpha;      /* [1,H,W] or NULL (= zeros) */
    const void* geom_buffer;
    const void* image_buffer;
    const uint32_t* point_list;
    const void* sorted_rec;      /* from forward */
    const void* quad_list;       /* from forward */
    void* bwd_tmp;               /* ogs_raster_backward_tmp_bytes(P): zeroed by the call (unless bwd_tmp_is_clear).  P * 16 must stay below 2^32 (the blend
                                    kernels address the record array with 32-bit element offsets): P < 2^28 = 268 M Gaussians,
                                    larger P is rejected with OGS_ERR_UNSUPPORTED.  Holds the per-Gaussian gradient
                                    record, 16 fp64 running sums = 128 B (float atomics arrive in a different order every
                                    run; an fp64 sum is order-insensitive to ~1e-16 and is rounded to fp32 once).  A features-only
                                    pass uses the first P * 64 bytes only: a record is then the <= 8 feature sums alone. */
    float* dL_dmeans2D;          /* [P,3] (x,y in NDC units: pixel gradient * 0.5*W / 0.5*H; z = 0) */
    float* dL_dcolors;           /* same shape as colors_precomp: [P,C], or [P,C-3] in a fused SH pass */
    float* dL_dopacity;          /* [P] */
    float* dL_dmeans3D;          /* [P,3] */
    float* dL_dcov3D;            /* [P,6]   (when cov3D_precomp was the input) */
    float* dL_dsh;               /* [P,M,3] (when shs was the input) */
    float* dL_dscales;           /* [P,3] */
    float* dL_drotations;        /* [P,4] */
    int32_t num_groups;          /* as in the forward pass (0/1: ungrouped): dL_dcolor is [G,C,H,W], dL_ddepth /
                                    dL_dalpha / out_alpha [G,1,H,W] */
    float* dL_dsh_rgb;           /* [P,3] optional (shs input only): gradient w.r.t. the SH-evaluated RGB after the
                                    clamp mask, zero for culled Gaussians.  Per view dL/dsh[p,m,:] = Y_m(dir(p)) *
                                    dL_dsh_rgb[p,:] (rank 1), so a data-parallel caller can pass dL_dsh = NULL,
                                    exchange these 3 floats instead of 3*M and rebuild the sum over views with
                                    ogs_sh_grad_from_views().  dL_dmeans3D still includes the view-direction term. */
    int32_t bwd_tmp_is_clear;    /* != 0: the caller vouches that the bytes of bwd_tmp this pass uses (P * 128, or P * 64 in a
                                    features-only pass with at most 8 feature sums) are zero already -- OgsRasterFwdArgs.bwd_clear
                                    of the forward, and nothing wrote them since -- and the call skips its fill.  0: the call
                                    clears them (the behaviour without this field). */
    /* Camera gradients (optional; no reference counterpart: the reference treats the camera as a constant).  For the loss L of
     * this pass (dL_dcolor, dL_ddepth, dL_dalpha) the partial derivatives of L with respect to the three camera arrays AS THE
     * KERNELS READ THEM, each array treated as independent of the other two:
     *   dL_dviewmatrix [16], in the storage order of `viewmatrix` (p_view.x = V[0] x + V[4] y + V[8] z + V[12], ...): depth through
     *       the z row, cov2D through the translation and through the rotation block (T = J W); entries 3, 7, 11, 15 are never read
     *       by a pass and are written as exact 0.0f;
     *   dL_dprojmatrix [16]: the pixel position through the hx, hy, hw rows, p_w = 1 / (hw + 1e-7f) differentiated as written;
     *       entries 2, 6, 10, 14 are exact zeros;
     *   dL_dcampos [3]: the view direction (mean - campos, normalised) of the SH colours, the clamp mask respected; exact zeros in
     *       a colors_precomp pass.
     * The paths are those dL_dmeans3D takes.  Cull, skip and saturation decisions are constants, culled and untouched Gaussians
     * contribute nothing, and where the +-1.3 tanfov clamp of tx/tz, ty/tz is active the clamped branch is detached (SURVEY.md
     * A.5).  Any parametrisation of the camera (an se(3) delta, full_proj = view @ P, campos = view.inverse()[3, :3]) is a chain
     * rule over these 35 numbers.  Every entry is an fp64 sum, in a fixed order, of one fp32 term per Gaussian, rounded once: two
     * calls on the same state give the same bits, and |error| stays within fp32 rounding of sum |term|.
     * All three NULL: the call is what it is without these fields -- the same launches, the same bytes.  Any one non-NULL: all
     * three and pose_tmp must be given (else OGS_ERR_INVALID_ARG), num_groups must be <= 1 (else OGS_ERR_UNSUPPORTED), the pass is
     * never the features-only one, and two launches follow the per-Gaussian backward on the same stream; all 35 floats are written
     * on every such call (P == 0, or a view that culls everything: zeros).  The per-Gaussian outputs may then ALL be NULL (a frozen
     * model whose pose trains): the full blend backward runs and only the 35 floats are written.  Not differentiated: tanfovx /
     * tanfovy / the image size. */
    float* dL_dviewmatrix;
    float* dL_dprojmatrix;
    float* dL_dcampos;
    void* pose_tmp;              /* ogs_raster_backward_pose_tmp_bytes(P): one row of partial sums per 256 Gaussians, every row
                                    written by the call (no clear needed) */
} OgsRasterBwdArgs;

int ogs_version(void);
const char* ogs_last_error(void);

/* Sticky asynchronous device status.  The one-launch radix passes (sorts of <= 256 k keys) wait for each other by decoupled
 * look-back; every wait is bounded, and a workgroup whose wait runs out ORs a bit into a word in pinned host memory, finishes
 * without hanging and without writing out of bounds, and leaves a WRONG permutation behind.  The library reads and clears the
 * word wherever the host already waits for the stream -- the blocking num_rendered read-back of ogs_raster_forward_geometry,
 * the entry of every later ogs_raster_forward_geometry / ogs_raster_backward -- and returns OGS_ERR_DEVICE; a caller of the
 * sync-free sequence (ogs_raster_read_num_rendered_async + _deferred) calls this after its own wait for the copy.  Returns
 * OGS_OK when nothing was reported since the last check.  (No reference counterpart: cub's sort has no failure mode that
 * returns.) */
int ogs_check_async_status(void);

size_t ogs_raster_geom_bytes(int32_t P, int32_t C);
size_t ogs_raster_geom_tmp_bytes(int32_t P);
size_t ogs_raster_image_bytes(int32_t W, int32_t H);
size_t ogs_raster_image_bytes_grouped(int32_t W, int32_t H, int32_t num_groups);
size_t ogs_raster_binning_tmp_bytes(int64_t num_rendered, int32_t W, int32_t H);
size_t ogs_raster_backward_tmp_bytes(int32_t P);
size_t ogs_raster_backward_pose_tmp_bytes(int32_t P);      /* OgsRasterBwdArgs.pose_tmp */
/* Test hook: how many per-workgroup rows of pose_tmp the second camera-gradient launch adds per step. */
int ogs_pose_partial_chunk(void);
size_t ogs_raster_sorted_bytes(int64_t num_rendered, int32_t C);
size_t ogs_raster_quad_list_bytes(int64_t num_rendered);

/* Phase 1: fills radii + geom_buffer, leaves the depth keys and tile offsets (and, for grouped passes and P <= 1024, the
 * depth order) in geom_tmp, writes
 * num_rendered to *num_rendered_host (host memory) and returns after the stream has finished it
 * (the same blocking read-back the reference performs once per forward).
 * num_rendered_host == NULL: no read-back, no synchronisation (see the deferred variant below).  out_color / out_depth /
 * out_alpha are not touched by this phase and may be NULL (a statistics pass has none). */
int ogs_raster_forward_geometry(const OgsRasterFwdArgs* args, void* stream, int64_t* num_rendered_host);

/* Phase 2: needs args->point_list / binning_tmp / sorted_rec / quad_list sized for num_rendered.  Asynchronous. */
int ogs_raster_forward_render(const OgsRasterFwdArgs* args, int64_t num_rendered, void* stream);

/* Sync-free variant of the two calls above (removes the GPU idle gap of the read-back):
 *   ogs_raster_forward_geometry(args, stream, NULL)            no copy, no synchronisation
 *   ogs_raster_read_num_rendered_async(args, stream, pinned)   enqueue the 4-byte D2H copy into PINNED host memory
 *   ogs_raster_forward_render_deferred(args, capacity, stream) buffers sized for `capacity` (e.g. 1.25x the last
 *        num_rendered); the binning kernels read the true count from device memory, entries past the capacity
 *        are dropped; a true count of ZERO is fine (background image, empty ranges)
 * The caller waits for the copy (an event recorded after it), and if *pinned > capacity re-runs
 * ogs_raster_forward_render with exact buffers -- the only case in which the deferred images are incomplete. */
int ogs_raster_read_num_rendered_async(const OgsRasterFwdArgs* args, void* stream, uint32_t* host_pinned);
int ogs_raster_forward_render_deferred(const OgsRasterFwdArgs* args, int64_t capacity, void* stream);

/* Diagnostics: how many (Gaussian, tile) pairs the render phase of this pass expands, read back with a BLOCKING 4-byte copy into
 * *host.  num_rendered stays the sum of the reference's tile rects (what the buffers are sized from); an ungrouped default-mode
 * pass of more than 1024 Gaussians expands each Gaussian's rect cut down to the bounding box of the ellipse inside which it can
 * reach alpha >= 1/255, so its count is smaller.  Every other pass: num_rendered.  Valid after ogs_raster_forward_geometry on the
 * same args while geom_tmp is alive. */
int ogs_raster_read_num_emitted(const OgsRasterFwdArgs* args, void* stream, uint32_t* host);

/* Tiny pass: the whole forward in TWO launches for P <= ogs_raster_tiny_max_points() Gaussians (ungrouped) -- the
 * single-Gaussian footprint renders of the SAM refiner (utils/sam_refinement_utils.py:330-403: one P = 1 call per
 * Gaussian and camera, thousands of times) and other very small subset renders, where the ~25 launches of the
 * streaming path are pure launch latency.  One workgroup preprocesses and depth-sorts every Gaussian; one workgroup
 * per tile then collects the Gaussians whose tile rect covers it (the reference's tile list, in its order) and blends
 * them.  Same images, radii, depth and alpha as the two-phase path, bit for bit.  Needs out_*, radii, geom_buffer
 * and geom_tmp; image_buffer / point_list / binning_tmp / sorted_rec / quad_list are not used and nothing is kept
 * for a backward pass (a caller that needs gradients re-renders through the two-phase path).  Asynchronous, no
 * read-back. */
size_t ogs_raster_tiny_max_points(void);
int ogs_raster_forward_tiny(const OgsRasterFwdArgs* args, void* stream);

/* List-length limits of the render phase's per-tile depth sort (test hook for their boundaries; no effect on results):
 * level 0: the longest list one wave sorts alone; level 1: the longest list a workgroup sorts in LDS (longer lists take
 * passes through global memory); level 2: the bucket cap in force (below); 0 for any other level. */
size_t ogs_raster_tile_sort_capacity(int32_t level);
/* A one-wave list is cut into buckets on its top differing key bits and every entry ranked inside its bucket; a list whose
 * largest bucket holds more than the bucket cap takes stable radix passes instead.  Same lists either way (test hook; no effect
 * on results): bucket_cap > 0 forces the cap, 0 hands the choice back to the library, a negative value leaves it as it is.
 * Process-wide.  Returns OGS_OK. */
int ogs_raster_tile_sort_debug(int32_t bucket_cap);

/* The counting sort by tile of a default streaming pass (test hooks; no effect on results).  The emitted pairs are cut into B
 * chunks, each a multiple of ogs_raster_tile_count_trip() pairs long.  ogs_raster_tile_count_debug returns the B a pass with a
 * list capacity D (the num_rendered, or the capacity, given to the render phase) and `tiles` tiles takes, 0 when it takes the
 * radix sort instead, after setting two process-wide hooks: force_blocks > 0 forces B (still cut to what the scratch has room
 * for: (B + 1) * tiles <= D), 0 hands the choice back; reverse != 0 places each chunk back to front (ties then arrive at the per-tile
 * depth sort in descending id order), 0 front to back.  A negative value leaves that hook as it is. */
int ogs_raster_tile_count_debug(int64_t D, int64_t tiles, int32_t force_blocks, int32_t reverse);
size_t ogs_raster_tile_count_trip(void);

/* The placement of that counting sort (test hooks; no effect on results).  Its grid is (place chunks) x (tile slices): a place
 * chunk is G consecutive chunks of the B above, a slice ceil(tiles / S) consecutive tiles, and a workgroup may stage its pairs in
 * up to stage_words words of LDS to write each tile's run in slot order; a workgroup with more pairs than that stores them one by
 * one.  group / slices / stage_words > 0 force G, S and the staging words (cut to what LDS has room for), 0 hands that choice back
 * to the library, a negative value leaves it as it is.  Process-wide.  chosen[0..2] (may be NULL) receives the place chunks
 * ceil(B / G), the slices and the staging words a pass with list capacity D and `tiles` tiles takes under the hooks as they
 * stand; all 0 when it takes the radix sort.  Returns OGS_OK. */
int ogs_raster_tile_place_debug(int64_t D, int64_t tiles, int32_t group, int32_t slices, int32_t stage_words, int32_t* chosen);

/* Re-blend of a KEPT pass (new capability; no reference counterpart -- the reference re-runs preprocess, both sorts and the
 * duplication on every call).  From stage 1 on the reference trains `_ins_feat` alone (train.py:431-436: every other Gaussian
 * parameter is detached) and renders without the random footprint rescale (train.py:346-350: rescale only in stage 2), so for a
 * given camera every later pass rebuilds, entry for entry, the binning state of the first one; only the feature channels of the
 * blended records differ.  A caller that kept image_buffer, sorted_rec and quad_list of a finished ungrouped pass (and its
 * radii) renders again with ONE launch: the forward blend walks the kept quadrant streams and takes channels [F0, C) of every
 * record from `colors_precomp` (by the Gaussian id the record carries) instead of the record -- images, depth, alpha, n_contrib
 * and final_T bit for bit what a full pass over the same inputs returns; the kept buffers are only read (n_contrib / final_T are
 * rewritten with the values they hold).  F0 = 3 and colors_precomp = [P, C-3] when the kept pass was a fused SH pass (flagged by sh_coeffs != 0: its
 * channels 0..2, the SH colours of the frozen coefficients for this camera, stay), else F0 = 0 and colors_precomp = [P, C].
 * Read: P, W, H, C, sh_coeffs, debug, bg, colors_precomp, out_color / out_depth / out_alpha, image_buffer, sorted_rec, quad_list;
 * everything else is ignored.  The caller owns the validity of the kept state: same means / scales / rotations / opacities / SH
 * coefficients, camera, image size, scale_modifier and binning mode as the kept pass (opengaussian_amd/rasterizer.py keys it on
 * the parameters' storage and version counters).  A features-only ogs_raster_backward on the kept state follows as after any
 * forward.  Asynchronous. */
int ogs_raster_forward_reblend(const OgsRasterFwdArgs* args, void* stream);

/* Compaction of the state a pass leaves behind, for a caller that keeps it (ogs_raster_forward_reblend).  The pass lays its
 * record array and quadrant streams out by the tile ranges of the sorted list -- tile t owns n_t = ranges[t].y - ranges[t].x slots
 * -- and packs only the k_t <= n_t records its pixels needed before every one of them was saturated (k_t = word 4 of the tile's
 * five counters in image_buffer; 15 % of the list on a ScanNet-class view).  The caller copies image_buffer, overwrites the
 * ranges at its start with new_ranges[t] = (exclusive scan of k, + k_t) -- image_buffer layout: uint2 ranges[tiles] first, then,
 * each 256-byte aligned, u32 n_contrib[W*H], u32 counters[tiles][5], float final_T[W*H], u32 tile_order[tiles] -- and this call
 * moves the k_t records and the four quadrant streams of every tile to the new offsets in buffers of
 * ogs_raster_sorted_bytes(sum k, C) / ogs_raster_quad_list_bytes(sum k).  The new triple (image, records, streams) is what
 * ogs_raster_forward_reblend and the features-only ogs_raster_backward take; ogs_raster_export_binning does not apply to it.
 * Asynchronous. */
int ogs_raster_compact_kept(int32_t W, int32_t H, int32_t C, const void* image_buffer, const void* sorted_rec,
                            const void* quad_list, void* new_image_buffer, void* new_sorted_rec, void* new_quad_list,
                            void* stream);

/* Grouped label statistics (new capability; no reference counterpart).  The 2D-3D association of the reference
 * (train.py construct_pseudo_ins_feat, stages 2.2 and 3) renders every cluster / leaf subset of a view and reads a few numbers
 * per (subset g, pseudo mask l) off the images: the pixels with alpha_g > thr inside mask l, the sum of subset g's blended colour
 * over them, and the maximum alpha of g.  The masks of one SAM level are disjoint, so one int32 label image carries them all and
 * those numbers are a histogram over it.  This pass is a grouped pass (OgsRasterFwdArgs.group_ids / num_groups) that takes the
 * histogram in the blend's epilogue instead of writing images: same preprocess, duplicate, sort, pack and blend, the same
 * per-pixel alpha and colour bit for bit, and nothing of size G*W*H allocated or written (no colour / depth / alpha images, no
 * n_contrib / final_T, no records or quadrant streams for a backward).
 *
 * Sequence: ogs_raster_forward_geometry(args, stream, &num_rendered) with args.out_color / out_depth / out_alpha == NULL allowed,
 * then this call with args.point_list / binning_tmp sized for num_rendered and args.image_buffer of
 * ogs_raster_stats_image_bytes(W, H, G); args.sorted_rec / quad_list are not used.  Outputs (cleared by the call):
 *   max_alpha [G] fp32        maximum over the image of group g's alpha (0 for a group without Gaussians);
 *   count     [G, L+1] int64  pixels with alpha > alpha_threshold, by label; bucket L = "no mask" (a label outside [0, L));
 *   feat_sum  [G, L+1, C] fp32 sum over those pixels of the blended colour INCLUDING the background term T * bg[c] -- the value
 *                             a grouped pass writes to out_color -- accumulated as int64 fixed point with a 2^-32 quantum
 *                             (order-independent: bit-reproducible run to run), rounded to fp32 once.  Exact to 2^-33 per
 *                             pixel; valid while |colour| * pixels < 2^31 (e.g. |colour| < 512 on 4 M pixels).
 * num_labels == 0 is legal (one bucket).  Asynchronous. */
typedef struct OgsGroupStatsArgs {
    const int32_t* labels;       /* [H*W] device: label of every pixel, -1 = no mask */
    int32_t num_labels;          /* L >= 0 */
    float alpha_threshold;       /* a pixel counts when alpha > alpha_threshold */
    float* max_alpha;            /* [G] */
    int64_t* count;              /* [G, L+1] */
    float* feat_sum;             /* [G, L+1, C] */
    void* stats_tmp;             /* ogs_raster_stats_tmp_bytes(G, L, C) */
} OgsGroupStatsArgs;

size_t ogs_raster_stats_image_bytes(int32_t W, int32_t H, int32_t num_groups);
size_t ogs_raster_stats_tmp_bytes(int32_t num_groups, int32_t num_labels, int32_t C);
int ogs_raster_forward_group_stats(const OgsRasterFwdArgs* args, const OgsGroupStatsArgs* stats, int64_t num_rendered,
                                   void* stream);

/* Backward.  Asynchronous on `stream`.  In the features-only case (see OgsRasterBwdArgs) only P, W, H, C, num_rendered,
 * num_groups, radii, dL_dcolor, image_buffer, sorted_rec, quad_list, bwd_tmp, dL_dcolors are read, `colors_precomp` and `shs`
 * are only tested against NULL (shs != NULL: fused SH pass, dL_dcolors is [P, C-3]); the other inputs, geom_buffer and
 * point_list may be NULL. */
int ogs_raster_backward(const OgsRasterBwdArgs* args, void* stream);

/* Replaces upstream mark_visible(means3D, viewmatrix, projmatrix) -> bool[P]: near-plane test
 * p_view.z > 0.2 (SURVEY.md section 2.1 `checkFrustum`). `present` is uint8[P]. */
int ogs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, void* stream);

/* Data-parallel helper (new capability; no reference counterpart): rebuilds
 *   dL_dsh[p,m,c] = sum_v Y_m((means3D[p] - campos[v]) / |.|) * dL_drgb[v,p,c]
 * i.e. the SUM over V views of the dL/dsh each view's backward would have written, from the per-view [P,3]
 * colour gradients (OgsRasterBwdArgs.dL_dsh_rgb, all-gathered over the ranks) and the V camera centres.
 * Exchanging 3 floats per Gaussian and view instead of all-reducing 3*M (48 at degree 3) cuts the xGMI bytes of
 * the SH gradient ~4x at 8 GPUs and fixes the summation order (v = 0..V-1), so the result is deterministic.
 * campos [V,3], dL_drgb [V,P,3], dL_dsh [P,sh_coeffs,3] (coefficients >= (sh_degree+1)^2 are written as 0). */
int ogs_sh_grad_from_views(int32_t P, int32_t V, int32_t sh_degree, int32_t sh_coeffs, const float* means3D,
                           const float* campos, const float* dL_drgb, float* dL_dsh, void* stream);

/* Test/diagnostic export of the binning state the reference keeps in its binningBuffer /
 * imgBuffer: the sorted 64-bit keys (tile << 32 | float_bits(depth)) [capacity num_rendered], the per-tile
 * ranges [T,2] and n_contrib [H,W].  Any output may be NULL.  The lists are those of the pass: after a pass with
 * args.full_binning != 0 the reference's full lists (num_rendered entries, n_contrib = position in the tile's full list);
 * after a default pass the reachable pairs only (max over the tiles of ranges[t].y entries; n_contrib = position in that shorter list). */
int ogs_raster_export_binning(const OgsRasterFwdArgs* args, int64_t num_rendered, uint64_t* keys_out,
                              uint32_t* ranges_out, uint32_t* n_contrib_out, void* stream);

/* Optional per-kernel timing with HIP events on the launch stream (used by bench.py's roofline leg;
 * not part of the reference boundary).  enable(1) starts a fresh recording of every launch, enable(2) of the
 * blend kernels only (two events per launch serialise the queue for ~10 us, so a timed region brackets only
 * the dominant kernels), enable(0) stops; collect() writes a JSON object
 * {"kernel": {"calls": n, "total_ms": t}, ...} into buf (host memory). */
int ogs_prof_enable(int on);
/* mode 2 brackets the kernels whose name starts with `prefix` (default "blend_"; at most 63 characters): a timed
 * region that only needs the dominant kernel's duration passes that kernel's name. */
int ogs_prof_filter(const char* prefix);
int ogs_prof_collect(char* buf, size_t n);

/* Test hook, not part of the reference boundary: runs the wave64 16-slot transposed reduction (mask reductions,
 * include/ogs_mask.h) on in[64][16]; out[lane] = sum over lanes of slot (lane >> 2). */
int ogs_selftest_wave_fold16(const float* in, float* out, void* stream);
/* Test hook: the accumulation step of the forward blend's walk as a matrix instruction (not used by the kernels: DESIGN.md section 3e).
 * One wave chains `steps` updates  acc[b][i][j] += w[t][16 b + i] * f[t][16 b + j]  (b < 4 blocks, i < 16 pixels, j < 16
 * channels; w, f: [steps][64]) starting from acc0 [4][16][16], once with the 4-block K = 1 fp32 MFMA (out_mfma, through the
 * accumulator layout written down in csrc/blend_fwd.hip) and once as one fmaf per element and step (out_fma).  The two must be
 * equal bit for bit. */
int ogs_selftest_mfma_rank1(const float* w, const float* f, const float* acc0, int32_t steps, float* out_mfma, float* out_fma,
                            void* stream);
/* Test hook: the heaviest-first workgroup order of the pack / blend kernels for tile ranges[vtiles][2] (start, end):
 * order[vtiles] = a permutation of the tiles, non-increasing in the length class of their lists -- or the identity
 * when the longest list is at most twice the mean (and for more than 65536 tiles). */
int ogs_selftest_tile_order(const uint32_t* ranges, int64_t vtiles, uint32_t* order, void* stream);
/* Test / measurement hook: the stable LSD radix sort of the binning phase on its own.
 * Sorts n (key, value) pairs on the low key_bits bits in ceil(key_bits / 8) passes, ping-ponging between buffers 0 and 1
 * (input in keys0 / vals0); *result_buffer (host) receives 0 or 1, the buffer pair holding the result.
 * variant bit 0 clear: three launches per pass (histogram table, row scan, scatter); set: one launch per pass (digit
 * histograms of all passes up front + decoupled look-back).  variant bit 1 set (n < 2^30): drop mode of the tile sort -- keys
 * equal to 0xFFFFFFFF are left out by the first pass, the result is the stable sort of the others and their count comes back in
 * bits 1.. of *result_buffer (bit 0: the buffer pair).  variant bit 2 set: fault injection -- the look-back waits of the
 * one-launch passes are bounded by zero polls, the call must return OGS_ERR_DEVICE.
 * items: keys per thread of a one-launch pass, 4 (1024-key tiles) or 16 (4096-key tiles); 0 = chosen by n as the library does.
 * n_dev (device, optional): the element count lives in device memory and n is the capacity the launches are sized for (the
 * deferred render phase); *n_dev == 0 is legal.  tmp: ogs_selftest_radix_tmp_bytes(n) bytes of scratch. */
size_t ogs_selftest_radix_tmp_bytes(int64_t n);
int ogs_selftest_radix_sort(uint32_t* keys0, uint32_t* vals0, uint32_t* keys1, uint32_t* vals1, int64_t n, int32_t key_bits,
                            int32_t variant, int32_t items, const uint32_t* n_dev, void* tmp, int32_t* result_buffer,
                            void* stream);
/* Test hook: the exclusive prefix sum every offset of the library comes out of (binning, densify, the kNN graph and index,
 * connected components), on its own.  out[i] = sum of the elements before i, modulo 2^32, for i < n; element i is in[i], or
 * in[gather[i]] when gather != NULL.  total (device, optional) receives the sum of all elements.  n_dev (device, optional): the
 * element count lives in device memory and n is the capacity the launches are sized for; the count is min(*n_dev, n), elements
 * past it count as zeros and their outputs are NOT written.  n <= 2048 is one launch, n <= 33 554 432 two, above that four
 * (five with total).  in may equal out, except with gather, and except with total above 33 554 432 elements: both return
 * OGS_ERR_INVALID_ARG before anything is launched or written, whatever n is (the gather refusal also for n <= 0).
 * Otherwise n <= 0: *total = 0, nothing else.
 * tmp: ogs_selftest_scan_tmp_bytes(n) bytes of scratch.  Asynchronous, no read-back. */
size_t ogs_selftest_scan_tmp_bytes(int64_t n);
int ogs_selftest_scan_u32(const uint32_t* in, const uint32_t* gather, uint32_t* out, int64_t n, uint32_t* total,
                          const uint32_t* n_dev, void* tmp, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OGS_RASTER_H */
