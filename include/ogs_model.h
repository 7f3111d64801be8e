/*
 * ogs_model.h -- the rasterizer pass taken from the model's RAW parameters.
 *
 * The reference's render() reads the model through torch getters (scene/gaussian_model.py:122-169) and the rasterizer
 * then sees activated copies; autograd carries the gradients back through the same graph.  The entry points below take
 * the raw parameters instead, apply the same activations inside the per-Gaussian kernels
 *
 *   scales    = exp(scaling)                         scene/gaussian_model.py:52,122-124    (torch.exp)
 *   rotations = rotation / max(|rotation|, 1e-12)    scene/gaussian_model.py:61,130-132    (F.normalize)
 *   opacities = 1 / (1 + exp(-opacity))              scene/gaussian_model.py:58,157-159    (torch.sigmoid)
 *   shs[:, 0] = features_dc, shs[:, 1:] = features_rest       scene/gaussian_model.py:151-155  (cat)
 *
 * and return gradients with respect to the raw parameters.  Everything else of a pass -- its buffers, its render phase
 * (ogs_raster_forward_render, _deferred, ogs_raster_read_num_rendered_async: they read only the per-Gaussian record),
 * the tiny / small / streaming choice -- is that of include/ogs_raster.h, and the results are bit for bit those of the
 * existing entry points fed with ogs_model_activate's outputs.
 *
 * All pointers are DEVICE pointers to contiguous fp32 data; `stream` is a hipStream_t passed as void*.
 */
#ifndef OGS_MODEL_H
#define OGS_MODEL_H

#include "ogs_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The reference model's parameters as GaussianModel stores them (scene/gaussian_model.py:67-72,202-206). */
typedef struct OgsRawModel {
    const float* features_dc;    /* [P,1,3] */
    const float* features_rest;  /* [P,M-1,3]; NULL when M == 1 */
    const float* scaling;        /* [P,3] log-scales */
    const float* rotation;       /* [P,4] unnormalised quaternions (r, x, y, z) */
    const float* opacity;        /* [P] logits */
} OgsRawModel;

/* Gradients with respect to the fields of OgsRawModel, same shapes.  Any pointer may be NULL (that family is skipped). */
typedef struct OgsRawModelGrads {
    float* features_dc;
    float* features_rest;
    float* scaling;
    float* rotation;
    float* opacity;
} OgsRawModelGrads;

/* ogs_raster_forward_geometry / ogs_raster_forward_tiny from raw parameters: replaces get_scaling, get_rotation,
 * get_opacity, get_features (scene/gaussian_model.py:122-159) in front of the rasterizer call of
 * gaussian_renderer/__init__.py:104-112.  args->sh_coeffs = M, args->C in {3, 6, 9, 12} with the C - 3 extra channels in
 * args->colors_precomp (C == 3: NULL).  args->shs, opacities, scales, rotations and cov3D_precomp must be NULL (the
 * raw model takes their place), features_rest may be NULL only when M == 1: anything else returns OGS_ERR_INVALID_ARG.
 * The render phase that follows is the existing one; it checks its arguments like every forward call, so hand it the same
 * struct with shs = raw->features_dc (non-NULL means "channels 0..2 come from SH", nothing is read through it), and
 * opacities / scales / rotations = the raw arrays (not read either). */
int ogs_raster_forward_geometry_raw(const OgsRasterFwdArgs* args, const OgsRawModel* raw, void* stream,
                                    int64_t* num_rendered_host);
int ogs_raster_forward_tiny_raw(const OgsRasterFwdArgs* args, const OgsRawModel* raw, void* stream);

/* ogs_raster_backward from raw parameters: replaces the autograd backward of the four getters above
 * (ExpBackward, DivBackward / NormBackward / ClampMinBackward of F.normalize, SigmoidBackward, CatBackward).
 * In args, shs / opacities / scales / rotations / cov3D_precomp and dL_dsh / dL_dopacity / dL_dscales / dL_drotations /
 * dL_dcov3D must be NULL: the inputs come from `raw`, those gradients go to `grads`.  dL_dmeans2D, dL_dmeans3D, dL_dcolors
 * ([P,C-3]) and dL_dsh_rgb keep their meaning.  grads->features_rest rows above the active degree, and every row of a
 * culled or untouched Gaussian, are written as zeros.  `grads` may be NULL (no raw gradient wanted: e.g. the features-only
 * pass, which is chosen exactly as in ogs_raster_backward). */
int ogs_raster_backward_raw(const OgsRasterBwdArgs* args, const OgsRawModel* raw, const OgsRawModelGrads* grads,
                            void* stream);

/* The four getters as one kernel: scales [P,3], rotations [P,4], opacities [P], shs [P,M,3] (scene/gaussian_model.py:122-159)
 * through the device functions the raw passes use -- for a caller that needs the activated arrays anyway, and for holding the
 * raw pass against the existing one.  Any output may be NULL (then its inputs may be NULL too). */
int ogs_model_activate(int32_t P, int32_t M, const OgsRawModel* raw, float* scales, float* rotations, float* opacities,
                       float* shs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OGS_MODEL_H */
