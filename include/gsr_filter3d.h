/*
 * gsr_filter3d.h -- the 3D smoothing filter of Mip-Splatting ("Mip-Splatting: Alias-free 3D Gaussian Splatting"), the half of the
 * method that antialiasing (gsr_aa.h, the screen-space filter) leaves out: a per-Gaussian low-pass radius derived from the closest
 * training camera that sees the Gaussian (GaussianModel.compute_3D_filter), folded into the scales and the opacity before every
 * render (get_scaling_with_3D_filter / get_opacity_with_3D_filter), into the opacity reset, and into the leaves a viewer loads
 * (save_fused_ply).  Entry points beside the core ABI of gsr.h, whose declarations they leave as they are.  When the filter is
 * recomputed stays with the caller.
 *
 * All float arrays are float32 on the device, laid out as the optimiser's leaves (fused_params): xyz [P][3], opacity logits [P][1],
 * log-scales [P][3], filter [P][1].  P < 2^31 / 3.
 *
 * gsr_filter3d_compute -- the camera sweep, three launches, no read-back, no atomics:
 *   camera c (gsr_filter3d_camera): p = R x + t (R row-major, world to camera), pixel = (p_x / p_z fx + cx, p_y / p_z fy + cy)
 *   valid_c = p_z > 0.2  and  -0.15 W <= pixel_x <= 1.15 W  and  -0.15 H <= pixel_y <= 1.15 H
 *   d_i     = min over the cameras valid for Gaussian i of p_z            (per_camera: of p_z / fx_c, the paper's sampling rate)
 *   rows valid in no camera take the largest d of the rows that are valid in one
 *   filter  = (d / f_max) * fp32(sqrt(0.2)),  f_max = max_c fx_c           (per_camera: d * fp32(sqrt(0.2)))
 * The frustum test is evaluated without the quotient, as p_x fx >= (-0.15 W - cx) p_z and so on (p_z > 0.2 there): the same set but
 * for rows that lie within fp32 rounding of a bound.  Where no row is valid in any camera every row of filter holds 100000, the
 * stock code's initial distance, as it stands (the stock code raises there; this form needs no read-back).
 * (1) one thread per Gaussian walks all C cameras -- every lane of a wave reads the same record, a wave-uniform address -- writes
 * d_i (0 for a row that is valid nowhere) to filter and its workgroup's largest d to scratch; (2) one workgroup folds those maxima
 * and forms f_max; (3) one thread per Gaussian writes the filter.  min and max do not depend on order: the result is bitwise
 * reproducible and the same bits under any permutation of the cameras.  scratch: gsr_filter3d_scratch_bytes(P) bytes, contents
 * irrelevant, free for reuse once the call's work on the stream has finished.
 *
 * gsr_filter3d_activate -- one launch, 20 B read and 16 B written per Gaussian.  With s_k = exp(log_scale_k), f = filter:
 *   scales_k  = sqrt(s_k^2 + f^2)
 *   coef      = prod_k s_k / sqrt(s_k^2 + f^2)
 *   opacities = sigmoid(logit) * coef
 * coef is formed per axis, never as sqrt(det / det'), whose numerator underflows in fp32 for small Gaussians and sends NaN through
 * the backward of the stock sequence.  Everything is evaluated in double precision from the float32 inputs and rounded once:
 * finite leaves with exp(log_scale) finite and f > 0 give finite outputs that underflow smoothly to 0.  An output pointer may be
 * NULL and is then not written.
 *
 * gsr_filter3d_activate_backward -- one launch, 36 B read and 16 B written per Gaussian; it recomputes the forward's values, so the
 * forward saves nothing but its three inputs.  With a_k = s_k^2, b_k = a_k + f^2:
 *   dL_dopacity   = g_o sigmoid(l) sigmoid(-l) coef                        (sigmoid(l) sigmoid(-l) from one exponential of -|l|)
 *   dL_dscaling_k = g_s,k a_k / sqrt(b_k) + g_o opacities f^2 / b_k
 * g_o = dL_dopacities [P][1], g_s = dL_dscales [P][3]; either may be NULL and counts as zero.  Either output may be NULL and is then
 * not written.  filter is a buffer and gets no gradient.
 *
 * gsr_filter3d_bake -- the forward's kernel in its other output mode: logit(opacities) and log(scales_k), the leaves for a viewer that
 * does not know the filter, in double and rounded once.  1 - opacities is formed as sigmoid(-l) + sigmoid(l) (1 - coef).
 *
 * gsr_filter3d_reset_opacity -- one launch, in place: logit <- logit(min(sigmoid(l), max_opacity / coef)), which is
 * logit(min(sigmoid(l) coef, max_opacity) / coef).  A row whose sigmoid(l) is at or below the cap keeps its bits (it is not sent
 * through sigmoid and logit); the others get the value evaluated in double and rounded once.  exp_avg and exp_avg_sq [P], given
 * together or both NULL, become +0.0 in every row.
 *
 * Refused with GSR_ERR_INVALID_ARGUMENT before any device work, with a message that starts with the function's name: a NULL
 * required pointer; P < 1; C < 1; one moment without the other; max_opacity outside (0, 1); 3 P beyond 2^31 - 1 (the kernels index
 * with 32 bits); every output of a call NULL.
 * Profiling stages (gsr_profile_*): "filter3d_sweep", "filter3d_activate", "filter3d_activate_bwd", "filter3d_reset".
 */
#ifndef GSR_FILTER3D_H_INCLUDED
#define GSR_FILTER3D_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_FILTER3D_THREADS 256            /* workgroup size of every kernel */
#define GSR_FILTER3D_CAMERA_FLOATS 20       /* sizeof(gsr_filter3d_camera) / 4 */
#define GSR_FILTER3D_UNSEEN 100000.0f       /* the filter of every row where no row is valid in any camera */

typedef struct gsr_filter3d_camera {
    float R[9];                 /* world to camera, row-major: p = R x + t */
    float t[3];
    float fx, fy, cx, cy;       /* pixels; the stock code centres at W / 2, H / 2 */
    float W, H;
    float pad[2];
} gsr_filter3d_camera;

size_t gsr_filter3d_scratch_bytes(int P);   /* 0 for a size that is not valid */
int gsr_filter3d_compute(int P, int C, const float* xyz, const gsr_filter3d_camera* cameras /* [C] on the device */, int per_camera,
                         float* filter, void* scratch, void* stream);
int gsr_filter3d_activate(int P, const float* opacity, const float* scaling, const float* filter, float* opacities /* or NULL */,
                          float* scales /* or NULL */, void* stream);
int gsr_filter3d_activate_backward(int P, const float* opacity, const float* scaling, const float* filter,
                                   const float* dL_dopacities /* or NULL */, const float* dL_dscales /* or NULL */,
                                   float* dL_dopacity /* or NULL */, float* dL_dscaling /* or NULL */, void* stream);
int gsr_filter3d_bake(int P, const float* opacity, const float* scaling, const float* filter, float* logits /* or NULL */,
                      float* log_scales /* or NULL */, void* stream);
int gsr_filter3d_reset_opacity(int P, float* opacity, const float* scaling, const float* filter, double max_opacity,
                               float* exp_avg /* or NULL */, float* exp_avg_sq /* or NULL */, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* GSR_FILTER3D_H_INCLUDED */
