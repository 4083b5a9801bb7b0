/*
 * gsr_cam.h -- camera gradients in libgsr_hip.so (include/gsr.h): dL/dviewmatrix, dL/dprojmatrix and dL/dcampos of the function the
 * backward already differentiates with respect to the Gaussians.  An entry point beside the core ABI of gsr.h, the maps of gsr_aux.h
 * and the filter of gsr_aa.h, whose declarations and struct layouts it leaves as they are.
 */
#ifndef GSR_CAM_H_INCLUDED
#define GSR_CAM_H_INCLUDED
#include "gsr.h"
#include "gsr_aux.h"
#include "gsr_aa.h"
#ifdef __cplusplus
extern "C" {
#endif
/*
 * The three camera tensors are independent inputs, exactly as the kernels read them (flat index 4 c + r, the layout of gsr.h):
 *   viewmatrix  through the view-space point t = V mean (the EWA Jacobian, the depth value of gsr_aux.h) and the rotation part W of
 *               T = W J; entries 4 k + 3 are exact zeros
 *   projmatrix  through the projected 2D mean; row 2 (entries 4 k + 2) reaches nothing differentiable: exact zeros
 *   campos      through the SH view direction; zeros when the colours were precomputed
 * with the backward's own conventions: the clamped t.x / t.y are constants inside J, and culling, radii, tile membership and depth
 * order carry no gradient.  tan_fovx / tan_fovy stay constants.
 *
 * The per-Gaussian pass sums the 27 non-zero terms over each wave of 64 Gaussians and stores one padded row of 32 floats per wave into
 * `scratch`; a second kernel folds the rows in a fixed order (no atomics: the same bits in every run) and writes all 35 outputs.
 *
 *   gsr_cam_bytes(P)   size of `scratch` for P Gaussians (never 0)
 *   gsr_cam_args       the outputs -- dL_dviewmatrix [16], dL_dprojmatrix [16], dL_dcampos [3], device memory -- and the scratch
 *                      (16-byte aligned; it need not be initialised and holds nothing afterwards)
 *
 * gsr_backward_gaussians_cam(args, antialiasing, opacities, aux, cam, first, count, out_row0): with cam == NULL it is
 * gsr_backward_gaussians_aa, argument for argument.  With cam it also produces the camera gradients and needs the whole scene in one
 * call, first == 0 and count == args->P: the part-by-part pipeline of view-parallel mode has no camera form.  The whole-backward calls
 * gsr_backward / gsr_backward_leaf have none either.
 */
typedef struct gsr_cam_args {
	float* dL_dviewmatrix;
	float* dL_dprojmatrix;
	float* dL_dcampos;
	void* scratch;
} gsr_cam_args;

size_t gsr_cam_bytes(int P);
int gsr_backward_gaussians_cam(const gsr_backward_args* args, int antialiasing, const float* opacities, const gsr_aux_args* aux,
                               const gsr_cam_args* cam, int first, int count, int out_row0);
#ifdef __cplusplus
}
#endif
#endif /* GSR_CAM_H_INCLUDED */
