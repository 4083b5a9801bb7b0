/*
 * gsr_cam_cm.h -- camera gradients under a camera model in libgsr_hip.so (include/gsr.h): dL/dviewmatrix, dL/dcampos and the gradient
 * of the model's intrinsics (fx, fy, cx, cy), of the function gsr_backward_gaussians_cm already differentiates with respect to the
 * Gaussians.  The camera-model form of gsr_cam.h: an entry point beside it and gsr_camera_model.h, whose declarations and struct
 * layouts it leaves as they are.
 */
#ifndef GSR_CAM_CM_H_INCLUDED
#define GSR_CAM_CM_H_INCLUDED
#include "gsr.h"
#include "gsr_aux.h"
#include "gsr_aa.h"
#include "gsr_camera_model.h"
#ifdef __cplusplus
extern "C" {
#endif
/*
 * Three independent inputs, exactly as the kernels read them:
 *   viewmatrix  (flat index 4 c + r) through the view-space point t = V mean -- the model's projection and Jacobian, the depth value
 *               of gsr_aux.h -- and the rotation part W of T = W J; entries 4 k + 3 are exact zeros
 *   campos      through the SH view direction; zeros when the colours were precomputed
 *   intrinsics  (fx, fy, cx, cy) of the gsr_camera_model, through the pixel mean and the Jacobian
 * with the backward's own conventions: inside the pinhole's guard band the clamped coordinate is a constant and the band's limits
 * carry no gradient with respect to the intrinsics; culling, radii, tile membership and depth order carry none.  There is no
 * projmatrix gradient: a model ignores that matrix.
 *
 * The per-Gaussian pass sums the 19 non-zero terms over each wave of 64 Gaussians and stores one padded row of 32 floats per wave
 * into `scratch`; a second kernel folds the rows in a fixed order (no atomics: the same bits in every run) and writes all
 * 16 + 4 + 3 outputs.
 *
 *   gsr_cam_cm_bytes(P)  size of `scratch` for P Gaussians (never 0)
 *   gsr_cam_cm_args      the outputs, device memory, and the scratch
 *
 * gsr_backward_gaussians_cam_cm(args, model, antialiasing, opacities, aux, cam, first, count, out_row0): with cam == NULL it is
 * gsr_backward_gaussians_cm, argument for argument.  With cam it needs a model, the whole scene in one call (first == 0 and
 * count == args->P), and non-NULL outputs and scratch.
 */
typedef struct gsr_cam_cm_args {
	float* dL_dviewmatrix;   /* [16] */
	float* dL_dintrinsics;   /* [4]: fx, fy, cx, cy */
	float* dL_dcampos;       /* [3] */
	void* scratch;           /* gsr_cam_cm_bytes(P), 16-byte aligned, need not be initialised */
} gsr_cam_cm_args;

size_t gsr_cam_cm_bytes(int P);   /* never 0 */
int gsr_backward_gaussians_cam_cm(const gsr_backward_args* args, const gsr_camera_model* model, int antialiasing, const float* opacities,
                                  const gsr_aux_args* aux, const gsr_cam_cm_args* cam, int first, int count, int out_row0);
#ifdef __cplusplus
}
#endif
#endif /* GSR_CAM_CM_H_INCLUDED */
