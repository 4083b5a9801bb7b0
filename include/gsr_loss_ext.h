/*
 * gsr_loss_ext.h -- the fused training loss of libgsr_hip.so (include/gsr.h, gsr_l1_ssim_loss) with the three things current 3DGS
 * training loops do around it: a per-pixel mask, a learnable per-image exposure (a 3x4 affine colour transform) and an L1 term on
 * the inverse-depth map against a prior.  An entry point beside the core ABI of gsr.h, whose declarations it leaves as they are;
 * gsr_l1_ssim_loss keeps its kernels.  Every option is optional and every combination is supported; the work stays one forward
 * kernel, one backward kernel and one fixed-order fold.
 *
 * All arrays are float32 on the device.  x = img [C][H][W], y = gt [C][H][W], m = mask [H][W] (values in [0, 1]; 1 without one),
 * E = exposure [3][4] row-major, d = invdepth [H][W], d* = invdepth_prior [H][W], k = invdepth_mask [H][W] (values >= 0; 1 without
 * one), w = invdepth_weight, l = lambda_dssim:
 *
 *   x'_c  = E[0][c] x_0 + E[1][c] x_1 + E[2][c] x_2 + E[c][3]                  (x' = x without exposure)
 *   x''   = m x',  y'' = m y
 *   L1    = mean over C, H, W of |x'' - y''|
 *   SSIM  = gsr_l1_ssim_loss's (11x11 window, sigma 1.5, fp32 taps, zero padding, C1 = 1e-4, C2 = 9e-4, mean over C H W) of x'', y'';
 *           the zero padding is of x'' and y'': outside the image both are 0, whatever E holds
 *   Ld    = mean over H, W of |(d - d*) k|                                     (0 without a depth term)
 *   vals  = {loss, L1, SSIM, Ld},  loss = (1 - l) L1 + l (1 - SSIM) + w Ld
 *
 * Gradients, each written in full where its pointer is not NULL, with G_c = m dloss/dx''_c:
 *   dL_dimg[k]         = sum_c E[k][c] G_c                                     (G_k without exposure)
 *   dL_dexposure[k][c] = sum over pixels of G_c x_k  (k < 3),   dL_dexposure[c][3] = sum over pixels of G_c       ([3][4] row-major)
 *   dL_dinvdepth       = w k sign((d - d*) k) / (H W)
 * The sign of 0 is 0.  A pixel with m == 0 has dL_dimg == +0.0 in every channel, one with k == 0 has dL_dinvdepth == +0.0.  gt, the
 * masks and the prior receive no gradient.
 *
 * No atomics anywhere: the value sums and the twelve exposure sums are taken per workgroup in a fixed order and folded by one
 * workgroup in a fixed order in double precision, so every output is bitwise reproducible run to run.  invdepth_weight travels by
 * value (a schedule in the caller's loop costs neither a synchronisation nor a recompilation).  `scratch`:
 * gsr_loss_ext_scratch_bytes(C, H, W) bytes, contents irrelevant, free for reuse once the call's work on the stream has finished.
 *
 * Refused with GSR_ERR_INVALID_ARGUMENT before any device work, with a message that starts with "gsr_l1_ssim_loss_ext:": NULL args;
 * a size that is not positive; NULL img, gt, vals or scratch; exposure with C != 3; dL_dexposure without exposure; exactly one of
 * invdepth / invdepth_prior; invdepth_mask or dL_dinvdepth without them; a negative or non-finite invdepth_weight.
 * Profiling stages (gsr_profile_*): "ssim_ext_forward", "ssim_ext_backward".
 */
#ifndef GSR_LOSS_EXT_H_INCLUDED
#define GSR_LOSS_EXT_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct gsr_loss_ext_args {
    int C, H, W;
    float lambda_dssim;
    const float *img, *gt;                                    /* [C][H][W] */
    const float *mask;                                        /* [H][W] or NULL */
    const float *exposure;                                    /* [3][4] row-major, device, or NULL; needs C == 3 */
    const float *invdepth, *invdepth_prior, *invdepth_mask;   /* [H][W]; the first two both or neither; the mask or NULL */
    float invdepth_weight;
    float *vals;                                              /* [4] loss, l1, ssim, depth_l1 */
    float *dL_dimg, *dL_dexposure, *dL_dinvdepth;             /* [C][H][W], [3][4], [H][W]; each or NULL */
    void *scratch, *stream;
} gsr_loss_ext_args;

size_t gsr_loss_ext_scratch_bytes(int C, int H, int W);       /* 0 for a size that is not positive */
int gsr_l1_ssim_loss_ext(const gsr_loss_ext_args* args);
#ifdef __cplusplus
}
#endif
#endif /* GSR_LOSS_EXT_H_INCLUDED */
