/*
 * gsr_features.h -- K per-Gaussian feature channels blended by the weights of a colour pass that already ran, with gradients, in
 * libgsr_hip.so (include/gsr.h): what semantic / language fields, normal maps and per-Gaussian scalars ask of a rasterizer.  Entry
 * points beside the core ABI of gsr.h, whose declarations and struct layouts they leave as they are.
 */
#ifndef GSR_FEATURES_H_INCLUDED
#define GSR_FEATURES_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
/*
 * With w_i(p) = alpha_i(p) T_i(p) the weight the forward blend multiplied Gaussian i's colour by at pixel p (0 where it did not blend):
 *   out[k][p] = sum_i features[i][k] w_i(p)          k = 0 .. K - 1, accumulated in list order with one FMA per term
 * There is no background term (add (1 - A) bg_k from the alpha map if wanted).  Every w has the forward's own bits, so channel k is
 * bit for bit the colour channel a forward with a zero background and the colour features[.][k] would have produced.  K >= 1 is
 * arbitrary (at most 262140); the channels are processed four at a time.
 *
 * gsr_features_forward reads the three state buffers as gsr_forward_render (of any variant: default, leaf, gsr_aux.h, gsr_aa.h)
 * left them, with the same P, num_rendered, width and height, and writes none of them.  `out` is written in full: zeros where nothing
 * blends, and for num_rendered == 0 by a fill alone.  debug: GSR_DEBUG_SYNC and GSR_DEBUG_NO_CULL are honoured.
 *
 * gsr_features_backward takes the gsr_backward_args of the colour backward of the same forward (sizes, state buffers, stream, debug;
 * with into_slots = 1 also `scratch`), g = dL_dout [K][height][width], and produces
 *   dL_dfeatures[i][k] = sum_p w_i(p) g_k(p)          every element is written, zeros for a Gaussian without a hit
 * and, with into_slots = 1, adds the feature map's part of dL/dmean2D, dL/dconic and dL/dopacity -- through
 * dL/dalpha_i(p) = sum_k (features[i][k] - accum_rec_k) g_k(p) T_i(p), the reference's per-pixel arithmetic with a zero background --
 * into words 0..5 of the per-(Gaussian, tile) gradient slots in args->scratch.  It must then be called after gsr_backward_blend /
 * _aux / _abs on the same args and before the first gsr_backward_gaussians*, which chain the total of colour and features; the
 * absolute gradients (gsr_absgrad.h) stay the colour's.  With into_slots = 0 args->scratch is neither read nor written and no colour
 * backward is needed: features on a frozen scene.  Of args the call reads P, num_rendered, width, height, geometry, binning, image,
 * stream, debug and (into_slots = 1) scratch.  `scratch`: gsr_features_scratch_bytes(P, num_rendered, K) bytes, 16-byte aligned,
 * contents irrelevant (what needs clearing is cleared on the stream inside the call); free for reuse once the call's work on the
 * stream has finished.  Nothing is added atomically; results are bitwise reproducible.
 *
 * Negative sizes, K < 1 (or beyond the limit), into_slots other than 0 or 1, and, with P > 0, NULL or misaligned (16 bytes) state or
 * scratch, NULL features or outputs and num_rendered beyond 32 bits return GSR_ERR_INVALID_ARGUMENT before any device work, with a
 * message that starts with the function's name; P == 0 returns GSR_OK and launches nothing; num_rendered == 0 launches only what
 * zero-fills the outputs.  Profiling stages (gsr_profile_*): "features_forward", "features_backward_tiles", "features_backward_fold".
 */
size_t gsr_features_scratch_bytes(int P, int64_t num_rendered, int K);
int gsr_features_forward(int P, int64_t num_rendered, int width, int height, int K,
                         const void* geometry, const void* binning, const void* image,
                         const float* features /* [P][K] */, float* out /* [K][H][W] */,
                         void* stream, int debug);
/* after gsr_backward_blend / _aux / _abs on the same args, before gsr_backward_gaussians*: */
int gsr_features_backward(const gsr_backward_args* args, int K, const float* features,
                          const float* dL_dout /* [K][H][W] */, float* dL_dfeatures /* [P][K] */,
                          void* scratch, int into_slots);
#ifdef __cplusplus
}
#endif
#endif /* GSR_FEATURES_H_INCLUDED */
