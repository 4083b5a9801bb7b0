/*
 * gsr_absgrad.h -- absolute screen-space gradients (AbsGS, gsplat's `absgrad`) in libgsr_hip.so (include/gsr.h): the densification
 * statistic that does not cancel.  An entry point beside the core ABI of gsr.h and the maps of gsr_aux.h, whose declarations and
 * struct layouts it leaves as they are.
 */
#ifndef GSR_ABSGRAD_H_INCLUDED
#define GSR_ABSGRAD_H_INCLUDED
#include "gsr.h"
#include "gsr_aux.h"
#ifdef __cplusplus
extern "C" {
#endif
/*
 * With f_p = G dL/dG of pixel p, dx_p / dy_p the pixel's offsets from the projected mean and (a, b, c) the conic, the backward writes
 *   dL/dmean2D.x = 0.5 W sum_p f_p (a dx_p + b dy_p)        dL/dmean2D.y = 0.5 H sum_p f_p (c dy_p + b dx_p)
 * in which per-pixel terms of opposite sign cancel: a large Gaussian over fine detail never reaches a split threshold built on their
 * norm.  The quantity here takes the modulus per pixel, before any sum,
 *   abs_dL_dmean2D[g] = (0.5 W sum_p |f_p (a dx_p + b dy_p)|, 0.5 H sum_p |f_p (c dy_p + b dx_p)|)
 * over exactly the pixels of the signed sums (same hit tests, same contributor limit), in the units of dL/dmean2D (NDC).  f_p is the
 * variant's own: with map gradients (gsr_aux.h) their terms are inside it.  It exists only inside the backward blend, so the blend has
 * a variant that keeps it:
 *
 * gsr_backward_blend_abs(args, aux, absgrad): with absgrad == 0 it is gsr_backward_blend_aux(args, aux), or gsr_backward_blend(args)
 * when aux is NULL, argument for argument.  With absgrad == 1 the blend also leaves each (Gaussian, tile) instance's two sums of
 * moduli in two spare words of the instance's gradient slot in args->scratch; everything else it writes has the same bits.
 *
 * gsr_absgrad_fold(args, abs, first, count): after that blend and before args->scratch is reused -- before or after
 * gsr_backward_gaussians* -- adds the slots of every Gaussian of [first, first + count) in a fixed order (no atomics: the same bits
 * in every run) and
 *   abs->abs_dL_dmean2D           [P][2], overwritten for every Gaussian of the range: exact zeros for culled Gaussians and for those
 *                                 that blended nowhere.  Needs no initialisation.
 *   abs->stat_abs_gradient_accum  [P], += sqrt(x^2 + y^2) for the visible Gaussians of the range (radii > 0, the rule of the stat_*
 *                                 arrays of gsr_backward_args; args->radii NULL: tiles touched > 0); others untouched.
 * Either may be NULL, not both.  Of args it reads P, num_rendered, width, height, radii, geometry, binning, scratch, stream and
 * debug (GSR_DEBUG_SYNC).  A range outside [0, P], a NULL `abs`, two NULL outputs and -- with work to do -- NULL state return
 * GSR_ERR_INVALID_ARGUMENT before any launch; count == 0 or P == 0 returns GSR_OK and launches nothing.  With num_rendered == 0
 * the zeros are still written.  Profiling stage (gsr_profile_*): "absgrad_fold"; the blend's stage keeps its name.
 */
typedef struct gsr_absgrad_args {
	float* abs_dL_dmean2D;
	float* stat_abs_gradient_accum;
} gsr_absgrad_args;

int gsr_backward_blend_abs(const gsr_backward_args* args, const gsr_aux_args* aux, int absgrad);
int gsr_absgrad_fold(const gsr_backward_args* args, const gsr_absgrad_args* abs, int first, int count);
#ifdef __cplusplus
}
#endif
#endif /* GSR_ABSGRAD_H_INCLUDED */
