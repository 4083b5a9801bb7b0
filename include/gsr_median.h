/*
 * gsr_median.h -- the median-depth map and the per-pixel Gaussian index maps of a forward, and the median depth's gradient, in
 * libgsr_hip.so (include/gsr.h): the depth map that surface extraction (TSDF fusion) consumes -- 2DGS, RaDe-GS, PGSR, gsplat's 2DGS
 * path -- and the per-pixel answer to "which Gaussian does this pixel see" that picking, mask lifting and keyframe bookkeeping ask of
 * a rasterizer.  Entry points beside the core ABI of gsr.h, whose declarations and struct layouts they leave as they are.
 */
#ifndef GSR_MEDIAN_H_INCLUDED
#define GSR_MEDIAN_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
/*
 * For pixel p take the Gaussians the forward blended into it, in list order, with T_i the transmittance in front of Gaussian i,
 * alpha_i its opacity at p and w_i = alpha_i T_i -- the forward's own values and accept / reject decisions, bit for bit:
 *   median(p)          = the LAST blended Gaussian with T_i > 0.5 (2DGS's `if (T > 0.5) median = this`, before T is updated).  The
 *                        first blended Gaussian has T = 1, so a pixel with a hit has a median; where T never falls to 0.5 it is the
 *                        last blended Gaussian.
 *   out_median_depth   = v of median(p), the value an aux-mode preprocess put into the splat record (view-space z for GSR_AUX_DEPTH,
 *                        1 / z for GSR_AUX_INVDEPTH), with the record's bits; 0 where nothing blends
 *   out_median_index   = the Gaussian id of median(p); -1 where nothing blends
 *   out_dominant_index = the id of the blended Gaussian with the largest w_i, the first in list order on a tie; -1 where nothing blends
 *   out_dominant_weight= that w_i, with the forward's bits; 0 where nothing blends
 *
 * gsr_median_forward reads the three state buffers as gsr_forward_render / _aux / _aa (packed or leaf) left them, with the same P,
 * num_rendered, width and height, and writes none of them.  Each output is [height][width]; any of the four may be NULL (not all) and
 * then costs nothing.  `state` -- one plane [height][width] of uint32, the median's position in its tile's list, 0xFFFFFFFF where
 * nothing blends; gsr_median_state_bytes(width, height) bytes, 16-byte aligned -- is what gsr_median_backward reads; it is required
 * with out_median_depth and may be NULL without it.  Everything requested is written in full, for num_rendered == 0 by fills alone
 * (0, -1, 0xFFFFFFFF).  After a forward without an aux mode the records hold v = 0, so out_median_depth is all zeros while the index
 * outputs and the weight are as valid as after an aux-mode forward.  debug: GSR_DEBUG_SYNC and GSR_DEBUG_NO_CULL are honoured, and
 * GSR_DEBUG_MEDIAN_FULL_WALK below.
 *
 * The kernel stops walking a band of the tile once none of its pixels can change: each has blended its last Gaussian, or has
 * T <= 0.5 (the median is fixed) and T <= the largest weight so far (w = alpha T <= T for alpha <= 0.99, so no later Gaussian wins
 * under the strict >).  The results are those of the full walk, bit for bit; GSR_DEBUG_MEDIAN_FULL_WALK runs the full walk.
 *
 * gsr_median_backward takes the gsr_backward_args of the colour backward of the same (aux-mode) forward, the state the forward call
 * wrote and g = dL_dmedian [height][width], and adds
 *   dL/dv_i = sum_{p : median(p) = i} g(p)
 * into word 9 of the per-(Gaussian, tile) gradient slots in args->scratch, the aux blend's own dL/dv.  The median depth is
 * differentiable in v only: the choice of i is piecewise constant, so nothing goes through alpha or T (as in 2DGS and gsplat).  It
 * must be called after gsr_backward_blend_aux (or gsr_backward_blend_abs with aux arguments) on the same args and before the first
 * gsr_backward_gaussians_aux / _aa / _cam with the same aux arguments, which chain the totals to dL/dmean3D along the view z axis, with
 * the -1 / z^2 of GSR_AUX_INVDEPTH -- the ordering contract of gsr_distortion_backward (gsr_distortion.h); the two may be called in
 * either order.  The median blended, so exactly slots the colour blend validated are updated.  Of args the call reads P, num_rendered,
 * width, height, geometry, binning, image, scratch, stream and debug.  Nothing is added atomically; every slot receives at most one
 * addition per call; results are bitwise reproducible.
 *
 * Negative sizes and, with P > 0, NULL or misaligned (16 bytes) state buffers, four NULL outputs, out_median_depth without state, a
 * NULL state / dL_dmedian in the backward and num_rendered beyond 32 bits return GSR_ERR_INVALID_ARGUMENT before any device work,
 * with a message that starts with the function's name; P == 0 returns GSR_OK and launches nothing; num_rendered == 0 launches only
 * what fills the forward's outputs (the backward: nothing).  Profiling stages (gsr_profile_*): "median_forward", "median_backward".
 */
#define GSR_DEBUG_MEDIAN_FULL_WALK 128 /* gsr_median_forward: no early exit, every band is walked to its last blended position */

size_t gsr_median_state_bytes(int width, int height);   /* 0 for a size that is not positive */
int gsr_median_forward(int P, int64_t num_rendered, int width, int height,
                       const void* geometry, const void* binning, const void* image,
                       float* out_median_depth, int32_t* out_median_index,
                       int32_t* out_dominant_index, float* out_dominant_weight,   /* [H][W] each; any NULL, not all */
                       void* state /* NULL allowed when out_median_depth is NULL */,
                       void* stream, int debug);
/* after gsr_backward_blend_aux on the same args, before gsr_backward_gaussians_aux: */
int gsr_median_backward(const gsr_backward_args* args, const void* state, const float* dL_dmedian /* [H][W] */);
#ifdef __cplusplus
}
#endif
#endif /* GSR_MEDIAN_H_INCLUDED */
