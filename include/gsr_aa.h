/*
 * gsr_aa.h -- anti-aliased rendering in libgsr_hip.so (include/gsr.h): the screen-space filter of Mip-Splatting, the reference
 * family's `antialiasing=True`.  Entry points beside the core ABI of gsr.h and the maps of gsr_aux.h, whose declarations and struct
 * layouts they leave as they are.
 */
#ifndef GSR_AA_H_INCLUDED
#define GSR_AA_H_INCLUDED
#include "gsr.h"
#include "gsr_aux.h"
#ifdef __cplusplus
extern "C" {
#endif
/*
 * The projected 2D covariance Sigma = [[a, b], [b, c]] is dilated by 0.3 px^2 on its diagonal in every path (conic, radius, tiles and
 * depth key are unchanged here).  With the filter on, the opacity is compensated for that dilation:
 *   N = a c - b^2,  Dh = (a + 0.3)(c + 0.3) - b^2,  rho = sqrt(max(2.5e-5, N / Dh))
 * and the splat record -- so the blend and the tile trim -- holds opacity * rho instead of the opacity.  A sub-pixel Gaussian then keeps
 * the footprint integral of its undilated self instead of growing by 1 / rho (about 4x at an isotropic sigma of 0.3 px).  The backward is
 * the exact derivative: dL/dopacity = dL/dopacity_record * rho, and dL/drho = dL/dopacity_record * opacity reaches dL/dcov3D (or
 * dL/dscale, dL/drot) and dL/dmean3D through the undilated entries.  With antialiasing = 0 every call is its default (aux == NULL) or
 * gsr_aux.h counterpart.
 *
 * A call sequence is all-anti-aliased or all-default:
 *   gsr_forward_preprocess_aa / gsr_forward_preprocess_leaf_aa   (aux: NULL, or the mode of gsr_aux.h's maps; only aux->mode is read)
 *   gsr_forward_render or gsr_forward_render_aux                  (unchanged: they read the record)
 *   gsr_backward_blend or gsr_backward_blend_aux                  (unchanged)
 *   gsr_backward_gaussians_aa                                     (aux: NULL, or the gsr_aux_args of gsr_backward_gaussians_aux)
 * The per-Gaussian backward needs the opacity INPUT, which the record no longer holds: `opacities` [P], the activated opacities of the
 * forward -- in leaf mode (args->leaf = 1) the opacity logits of gsr_forward_preprocess_leaf_aa.  first / count / out_row0 are those of
 * gsr_backward_gaussians.  The whole-backward calls gsr_backward / gsr_backward_leaf have no anti-aliased form.
 */
int gsr_forward_preprocess_aa(
	int antialiasing, const gsr_aux_args* aux,
	int P, int D, int M, int width, int height,
	const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
	const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
	const float* viewmatrix, const float* projmatrix, const float* cam_pos,
	float tan_fovx, float tan_fovy, int prefiltered,
	int* radii, void* geometry, int64_t* num_rendered_host, void* stream, int debug);
int gsr_forward_preprocess_leaf_aa(
	int antialiasing, const gsr_aux_args* aux,
	int P, int D, int M, int width, int height,
	const float* xyz, const float* features_dc, const float* features_rest,
	const float* opacity_logits, const float* log_scales, float scale_modifier, const float* raw_rotations,
	const float* viewmatrix, const float* projmatrix, const float* cam_pos,
	float tan_fovx, float tan_fovy, int prefiltered,
	int* radii, void* geometry, int64_t* num_rendered_host, void* stream, int debug);
int gsr_backward_gaussians_aa(const gsr_backward_args* args, int antialiasing, const float* opacities, const gsr_aux_args* aux,
                              int first, int count, int out_row0);
#ifdef __cplusplus
}
#endif
#endif /* GSR_AA_H_INCLUDED */
