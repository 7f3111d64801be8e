/*
 * ogs_loss.h -- C ABI of the full-frame image losses of OpenGaussian's stage 0 and stage 2.
 *
 * Replaces
 *   /root/reference/utils/loss_utils.py:33-73   gaussian / create_window / ssim / _ssim
 *   /root/reference/utils/loss_utils.py:17-31   l1_loss / l2_loss (plain and masked)
 *   /root/reference/train.py:385-386            (1 - lambda) * l1_loss + lambda * (1 - ssim)
 *   /root/reference/train.py:471, :483          l1_loss(.., keeped_pix), l2_loss(.., cluster_silhouette)
 * i.e. five depthwise 11x11 conv2d calls, ~15 full-frame elementwise kernels and their autograd twins (stage 0), ~8 + 8
 * full-frame kernels (stage 2), with one tiled kernel + one tiny reduce launch per direction.
 *
 * SSIM is the reference's: 11 taps, sigma 1.5, 1-D weights exp(-(i-5)^2 / (2 sigma^2)) normalised and rounded to fp32, the
 * 2-D window their outer product, ZERO padding of 5 (taps outside the image add 0, the weights are not renormalised),
 * moments G*x, G*y, G*x^2, G*y^2, G*xy, C1 = 0.01^2, C2 = 0.03^2, mean over all C*H*W.
 *
 * All pointers are DEVICE pointers; images are contiguous fp32 [C,H,W]; masks are bytes (0 = outside, anything else =
 * inside).  `stream` is a hipStream_t as void*.  Returns 0 or a negative OGS_ERR_* code (ogs_raster.h);
 * ogs_last_error() describes it.  Sums are reduced WITHOUT atomics: every workgroup writes one partial pair (fp64) into
 * `partials`, a second one-workgroup launch adds the pairs in index order in fp64 -- the result is the same bits from run to run.
 *
 * Algorithmic HBM bytes (N = C*H*W floats; tile halos are re-reads out of L2):
 *   photometric forward    reads img, gt                      8 N   writes 16 B per tile
 *   photometric backward   reads img, gt   writes dimg       12 N   (A, B, Cm are RECOMPUTED from img and gt; saving them in
 *                          forward would be 8 N + 12 N = 20 N forward and 20 N + 4 N = 24 N backward: 44 N against 20 N)
 *   masked forward         reads x, t (+ mask 1 B, weight 4 B per mask element)      8 N + (1|5) M
 *   masked backward        the same reads, writes dx                                12 N + (1|5) M
 */
#ifndef OGS_LOSS_H
#define OGS_LOSS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of `partials` scratch the photometric forward needs for a [C,H,W] image (one fp64 pair per tile and channel). */
size_t ogs_loss_photometric_tmp_bytes(int32_t C, int32_t H, int32_t W);

/* img, gt [C=3,H,W], any H, W >= 1.  out[5] (fp32, each the fp64 total rounded once):
 *   out[0] = sum |img - gt|          out[1] = sum ssim_map
 *   out[2] = out[0] / (C H W)        out[3] = out[1] / (C H W)              (l1_loss, ssim of the reference)
 *   out[4] = (1 - lambda_dssim) * l1 + lambda_dssim * (1 - ssim)            (train.py:385-386) */
int ogs_loss_photometric_forward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                                 float* out, void* partials, void* stream);

/* dimg [C,H,W] (every element written) for upstream scalars read from device memory, each pointer may be NULL (= 0):
 *   g_l1 = dL/d out[2], g_ssim = dL/d out[3], g_loss = dL/d out[4]; with gl = g_l1 + (1 - lambda) g_loss and
 *   gs = g_ssim - lambda g_loss:
 *   dimg = gs / (CHW) * (G*A + 2 img (G*B) + gt (G*Cm)) + gl / (CHW) * sign(img - gt),      sign(0) = 0
 * where A = d s / d mu_x (with the dependence of sigma_x^2 and sigma_xy on mu_x folded in), B = d s / d sigma_x^2,
 * Cm = d s / d sigma_xy at every pixel of the image, and G* is the same zero-padded filter (symmetric window, zero
 * padding: the filter is its own adjoint).  There is no gradient for gt. */
int ogs_loss_photometric_backward(const float* img, const float* gt, const float* g_l1, const float* g_ssim,
                                  const float* g_loss, float lambda_dssim, int32_t C, int32_t H, int32_t W, float* dimg,
                                  void* stream);

/* Bytes of `partials` scratch the masked forward needs (independent of the size: the grid is capped). */
size_t ogs_loss_masked_tmp_bytes(void);

/* x, t [C,HW], C = 3 or 6 (any C >= 1 when mask == NULL); p = 1 (L1) or 2 (L2).
 * mask: NULL, or bytes [HW] (mask_channels = 1, shared by the channels) or [C*HW] (mask_channels = C);
 * weight: NULL or fp32 of the mask's extent (needs a mask).  out[3]:
 *   out[0] = num = sum |(x - t) m w|  (p = 1)   or   sum (x - t)^2 m w  (p = 2)
 *   out[1] = sum m over the mask's OWN elements (a [HW] mask over 6 channels counts pixels, not 6 x pixels);
 *            C * HW when mask == NULL
 *   out[2] = out[0] / max(out[1], 1)                                    (l1_loss / l2_loss of the reference) */
int ogs_loss_masked_forward(const float* x, const float* t, const uint8_t* mask, const float* weight, int32_t mask_channels,
                            int32_t p, int32_t C, int64_t HW, float* out, void* partials, void* stream);

/* dx [C,HW] = g[0] * d out[2] / d x, every element written, exactly 0 outside the mask; `fwd_out` is the forward's out
 * (out[1] is read), g one fp32 on the device. */
int ogs_loss_masked_backward(const float* x, const float* t, const uint8_t* mask, const float* weight,
                             int32_t mask_channels, int32_t p, int32_t C, int64_t HW, const float* fwd_out, const float* g,
                             float* dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OGS_LOSS_H */
