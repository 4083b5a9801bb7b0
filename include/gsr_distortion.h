/*
 * gsr_distortion.h -- the depth-distortion map of a depth-and-alpha forward (include/gsr_aux.h) and its gradient, in libgsr_hip.so
 * (include/gsr.h): the per-ray spread of the blend weights along depth that geometry regularisers ask of a rasterizer (Mip-NeRF 360's
 * distortion loss in the pairwise squared form of 2DGS, gsplat's `distloss`).  Entry points beside the core ABI of gsr.h, whose
 * declarations and struct layouts they leave as they are.
 */
#ifndef GSR_DISTORTION_H_INCLUDED
#define GSR_DISTORTION_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
/*
 * With w_i(p) = alpha_i(p) T_i(p) the weight the forward blend multiplied Gaussian i's colour by at pixel p (0 where it did not blend)
 * and v_i the depth value an aux-mode preprocess put into the splat record (view-space z_i for GSR_AUX_DEPTH, 1 / z_i for
 * GSR_AUX_INVDEPTH):
 *   out_dist[p] = sum_{j<i} w_i w_j (v_i - v_j)^2  =  1/2 sum_i sum_j w_i w_j (v_i - v_j)^2
 * No background term; 0 where fewer than two Gaussians blend; symmetric, so independent of the list's order in v; invariant under
 * v -> v - c.  Every w has the forward's own bits.  The sum is evaluated centred, by a weighted Welford recurrence per pixel in list
 * order (A' = A + w, d = v - mu, mu' = mu + (w / A') d, S' = S + w d (v - mu'), out = A S), never from raw moments.
 *
 * gsr_distortion_forward reads the three state buffers as gsr_forward_render_aux (or _aa with an aux mode; packed or leaf) left them,
 * with the same P, num_rendered, width and height, and writes none of them.  out_dist [height][width] and `state` -- three planes
 * [3][height][width] of floats: A = sum w, mu = the weighted mean of v, S = sum w (v - mu)^2; gsr_distortion_state_bytes(width,
 * height) bytes, 16-byte aligned -- are written in full: zeros where nothing blends, and for num_rendered == 0 by fills alone.
 * After a forward without an aux mode the records hold v = 0 and the map is all zeros.  debug: GSR_DEBUG_SYNC and GSR_DEBUG_NO_CULL
 * are honoured.
 *
 * gsr_distortion_backward takes the gsr_backward_args of the colour backward of the same forward, the state the forward call wrote
 * and g = dL_ddist [height][width], and adds the map's part of the gradients into the per-(Gaussian, tile) gradient slots in
 * args->scratch: with h_i(p) = dDist/dw_i = A (v_i - mu)^2 + S,
 *   dL/dalpha_i(p) = T_i (g h_i - accum_rec)         accum_rec: the back-to-front blend of g h, zero background (gsr_features.h's
 *                                                    arithmetic with the per-pixel "feature" g h_i)
 * finished to dL/dmean2D, dL/dconic and dL/dopacity and added into words 0..5 of the slot, and
 *   dL/dv_i = sum_p 2 g w_i A (v_i - mu)             added into word 9, the aux blend's own dL/dv
 * It must be called after gsr_backward_blend_aux (or gsr_backward_blend_abs with aux arguments) on the same args and before the first
 * gsr_backward_gaussians_aux / _aa / _cam with the same aux arguments, which chain the totals -- word 9 to dL/dmean3D along the view z
 * axis, with the -1 / z^2 of GSR_AUX_INVDEPTH.  The hit set is the colour blend's, so exactly the slots it validated are updated; the
 * absolute gradients (gsr_absgrad.h) stay the colour's.  Of args the call reads P, num_rendered, width, height, geometry, binning,
 * image, scratch, stream and debug.  Nothing is added atomically; results are bitwise reproducible.
 *
 * Negative sizes and, with P > 0, NULL or misaligned (16 bytes) state buffers, a NULL out_dist / dL_ddist and num_rendered beyond 32
 * bits return GSR_ERR_INVALID_ARGUMENT before any device work, with a message that starts with the function's name; P == 0 returns
 * GSR_OK and launches nothing; num_rendered == 0 launches only what zero-fills the forward's outputs (the backward: nothing).
 * Profiling stages (gsr_profile_*): "distortion_forward", "distortion_backward".
 */
size_t gsr_distortion_state_bytes(int width, int height);   /* 0 for a size that is not positive */
int gsr_distortion_forward(int P, int64_t num_rendered, int width, int height,
                           const void* geometry, const void* binning, const void* image,
                           float* out_dist /* [H][W] */, void* state,
                           void* stream, int debug);
/* after gsr_backward_blend_aux on the same args, before gsr_backward_gaussians_aux: */
int gsr_distortion_backward(const gsr_backward_args* args, const void* state, const float* dL_ddist /* [H][W] */);
#ifdef __cplusplus
}
#endif
#endif /* GSR_DISTORTION_H_INCLUDED */
