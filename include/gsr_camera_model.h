/*
 * gsr_camera_model.h -- camera models in libgsr_hip.so (include/gsr.h): a pinhole with intrinsics (off-centre principal point) and an
 * equidistant fisheye.  Entry points beside the core ABI of gsr.h, the maps of gsr_aux.h and the filter of gsr_aa.h, whose
 * declarations and struct layouts they leave as they are.
 */
#ifndef GSR_CAMERA_MODEL_H_INCLUDED
#define GSR_CAMERA_MODEL_H_INCLUDED
#include "gsr.h"
#include "gsr_aux.h"
#include "gsr_aa.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_CAMERA_PINHOLE 0
#define GSR_CAMERA_FISHEYE 1
/*
 * fx, fy: focal lengths in pixels (finite, > 0).  cx, cy: the principal point in pixels, OpenCV / COLMAP convention -- origin at the
 * corner of the first pixel, pixel centres at +0.5 -- so the pixel-index coordinates of the splat record are
 *   u = (projected x) + cx - 0.5,  v = (projected y) + cy - 0.5.
 * The camera of the core ABI is {GSR_CAMERA_PINHOLE, W / (2 tan_fovx), H / (2 tan_fovy), W / 2, H / 2}.
 *
 * With t = viewmatrix * mean (view space; Gaussians with t.z <= 0.2 are culled as in the core ABI, the depth key and the depth value
 * of gsr_aux.h stay t.z, the SH direction stays mean - cam_pos):
 *   GSR_CAMERA_PINHOLE  u = fx t.x / t.z + cx - 0.5, v = fy t.y / t.z + cy - 0.5.  The EWA Jacobian is the core ABI's with fx, fy; its
 *                       guard band follows the principal point: t.x / t.z is clamped to
 *                       [-(cx / fx + 0.3 W / (2 fx)), (W - cx) / fx + 0.3 W / (2 fx)], t.y / t.z likewise with cy, fy, H (the core ABI's
 *                       +-1.3 tan_fov at its own intrinsics).  The clamp is a constant in the backward.
 *   GSR_CAMERA_FISHEYE  equidistant, no distortion coefficients: r = sqrt(t.x^2 + t.y^2), theta = atan2(r, t.z), s = theta / r,
 *                       u = fx s t.x + cx - 0.5, v = fy s t.y + cy - 0.5.  The Jacobian is the full 2x3 one of that map; no guard band.
 * Dilation, rho of gsr_aa.h, radius, tile rectangle and trim are those of the core ABI: they consume (u, v, covariance).
 *
 * projmatrix, tan_fovx and tan_fovy of the calls (and of gsr_backward_args) are ignored with a model; projmatrix may be NULL then.
 * dL_dmean2D keeps the core ABI's units (0.5 W dL/du, 0.5 H dL/dv).
 *
 * A call sequence uses one model throughout:
 *   gsr_forward_preprocess_cm / gsr_forward_preprocess_leaf_cm   (the *_aa forms of gsr_aa.h with the model in front)
 *   gsr_forward_render or gsr_forward_render_aux                  (unchanged: they read the record)
 *   gsr_backward_blend, gsr_backward_blend_aux, ...               (unchanged)
 *   gsr_backward_gaussians_cm                                     (gsr_backward_gaussians_aa with the model)
 * model == NULL: the call is its *_aa form.  The camera gradients of gsr_cam.h and the whole-backward calls have no such form.
 */
typedef struct gsr_camera_model {
	int model;      /* GSR_CAMERA_* */
	float fx, fy;
	float cx, cy;
} gsr_camera_model;

int gsr_forward_preprocess_cm(
	const gsr_camera_model* model, int antialiasing, const gsr_aux_args* aux,
	int P, int D, int M, int width, int height,
	const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
	const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
	const float* viewmatrix, const float* projmatrix, const float* cam_pos,
	float tan_fovx, float tan_fovy, int prefiltered,
	int* radii, void* geometry, int64_t* num_rendered_host, void* stream, int debug);
int gsr_forward_preprocess_leaf_cm(
	const gsr_camera_model* model, int antialiasing, const gsr_aux_args* aux,
	int P, int D, int M, int width, int height,
	const float* xyz, const float* features_dc, const float* features_rest,
	const float* opacity_logits, const float* log_scales, float scale_modifier, const float* raw_rotations,
	const float* viewmatrix, const float* projmatrix, const float* cam_pos,
	float tan_fovx, float tan_fovy, int prefiltered,
	int* radii, void* geometry, int64_t* num_rendered_host, void* stream, int debug);
int gsr_backward_gaussians_cm(const gsr_backward_args* args, const gsr_camera_model* model, int antialiasing, const float* opacities,
                              const gsr_aux_args* aux, int first, int count, int out_row0);
#ifdef __cplusplus
}
#endif
#endif /* GSR_CAMERA_MODEL_H_INCLUDED */
