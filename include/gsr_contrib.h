/*
 * gsr_contrib.h -- per-Gaussian blend-weight statistics of one view in libgsr_hip.so (include/gsr.h): what pruning, compaction and
 * error-based densification ask of a rasterizer.  An entry point beside the core ABI of gsr.h, whose declarations and struct layouts
 * it leaves as they are.
 */
#ifndef GSR_CONTRIB_H_INCLUDED
#define GSR_CONTRIB_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
/*
 * With w_g(p) = alpha_g(p) T_g(p) the weight the forward blend multiplied Gaussian g's colour by at pixel p (0 where it did not blend):
 *   weight_sum[g]  += sum_p m(p) w_g(p)      m = pixel_weight, [height][width], or 1 everywhere when it is NULL
 *   weight_max[g]   = max(weight_max[g], max_p w_g(p))
 *   pixel_count[g] += the number of pixels g blended into
 * for every Gaussian that blended into at least one pixel of the view; the others are left untouched (the convention of the stat_*
 * arrays of gsr_backward_args), so a sweep over views accumulates into the same arrays without further launches.  Any of the three
 * may be NULL, not all (with P > 0).  Every w is the forward's own value bit for bit, nothing is added atomically, and the result
 * is bitwise reproducible.
 *
 * The call reads the three state buffers as gsr_forward_render (of any variant: default, leaf, gsr_aux.h, gsr_aa.h -- with the
 * screen-space filter w contains the compensated opacity) left them, with the same P, num_rendered, width and height, and writes none
 * of them: it may run before or after the backward of that forward, which is unaffected.  `scratch`: gsr_contrib_scratch_bytes(P,
 * num_rendered) bytes, 16-byte aligned, contents irrelevant (what needs clearing is cleared on `stream` inside the call); free for
 * reuse once the call's work on `stream` has finished.  debug: GSR_DEBUG_SYNC and GSR_DEBUG_NO_CULL are honoured.
 *
 * Negative sizes and, with P > 0, NULL state, three NULL outputs, and NULL scratch with num_rendered > 0 return
 * GSR_ERR_INVALID_ARGUMENT before any device work; otherwise P == 0 or num_rendered == 0 returns GSR_OK and launches nothing.
 * Profiling stages (gsr_profile_*): "contrib_tiles", "contrib_gaussians".
 */
size_t gsr_contrib_scratch_bytes(int P, int64_t num_rendered);
int gsr_contributions(int P, int64_t num_rendered, int width, int height,
                      const void* geometry, const void* binning, const void* image,
                      const float* pixel_weight,
                      float* weight_sum, float* weight_max, int32_t* pixel_count,
                      void* scratch, void* stream, int debug);
#ifdef __cplusplus
}
#endif
#endif /* GSR_CONTRIB_H_INCLUDED */
