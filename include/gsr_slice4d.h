/*
 * gsr_slice4d.h -- 4D Gaussians rendered at a time stamp ("Real-time Photorealistic Dynamic Scene Representation and Rendering with 4D
 * Gaussian Splatting", Yang et al.): every primitive is a Gaussian over (x, y, z, t); for a frame at `time` it is conditioned on
 * t = time, which yields what the rasterizer already takes -- means3D, cov3D_precomp, opacities, shs.  Entry points beside the core
 * ABI of gsr.h, whose declarations they leave as they are.
 *
 * All float arrays are float32 on the device, contiguous, laid out as the optimiser's leaves (fused_params): xyz [P][3], t [P][1],
 * scaling [P][3] (log), scaling_t [P][1] (log), rotation [P][4] (raw l = (a,b,c,d)), rotation_r [P][4] (raw r = (p,q,r,s)),
 * opacity [P][1] (logit).  Quaternions are (w, x, y, z).  6 P < 2^31.
 *
 * The rule.  A 4-vector (x, y, z, t) is the quaternion t + x i + y j + z k.  With l^ = l / |l| and r^ = r / |r| the rotation is
 * R v = l^ v conj(r^); in the (x, y, z, t) ordering R = L(l^) M(r^) with
 *     L(a,b,c,d) = [  a -d  c  b ]      M(p,q,r,s) = [  p -s  r -q ]
 *                  [  d  a -b  c ]                   [  s  p -q -r ]
 *                  [ -c  b  a  d ]                   [ -r  q  p -s ]
 *                  [ -b -c -d  a ]                   [  q  r  s  p ]
 * R is orthogonal with determinant +1, L and M commute, every element of SO(4) is reached, and l = r gives blockdiag(R3(l), 1) with
 * R3 the 3D rotation of the quaternion l: the static limit.  A checkpoint trained with another parametrisation of the two quaternions
 * is converted by the caller.  With the time `time`, the scaling modifier m and the cutoff c:
 *     s_k       = m exp(log-scale_k), k = x, y, z, t;   Sigma = R diag(s^2) R^T
 *     Sigma_tt  = sum_k R_3k^2 s_k^2,   u_i = sum_k R_ik R_3k s_k^2 (i < 3),   velocity = u / Sigma_tt,   D = time - t
 *     means3D   = xyz + velocity D
 *     cov3D     = Sigma_11 - u u^T / Sigma_tt, stored (xx, xy, xz, yy, yz, zz): the rasterizer's cov3D_precomp
 *     g         = exp(-D^2 / (2 Sigma_tt))
 *     opacities = sigmoid(opacity) g where g > c, elsewhere exactly +0: the row is masked (c = 0.05 is the paper's rule)
 * Everything is evaluated in double precision from the float32 inputs and rounded once, so the difference
 * Sigma_11 - u u^T / Sigma_tt, whose result is up to 10^4 times smaller than its terms, loses nothing that float32 can hold.
 * Quaternions of norm zero and leaves that are not finite are the caller's business: the kernels stay in bounds and define no value.
 *
 * gsr_slice4d_forward -- one launch; 68 B read and 40 B written per Gaussian, 12 B more with velocity.  An output pointer may be
 * NULL and is then not written.
 *
 * gsr_slice4d_backward -- one launch; it recomputes the forward's values, so the forward saves nothing but its inputs.  dL_dmeans3D
 * [P][3], dL_dcov3D [P][6] (with respect to the six stored values, which is what autograd hands back for cov3D_precomp),
 * dL_dopacities [P][1], dL_dvelocity [P][3]: any may be NULL and counts as zero.  The seven leaf gradients have the leaves' shapes; any
 * may be NULL and is then not written.  The chain through R to both raw quaternions, both normalisations included, is written out
 * (csrc/gsr_slice4d_math.h).  Every leaf gradient of a masked row is exactly +0 whatever arrives, dL_dxyz included: 4DGS skips such a
 * Gaussian altogether.  `time` gets no gradient.
 *
 * gsr_harmonic_features -- colour coefficients modulated by a Fourier series in time - t.  features_t [P][N+1][M][3] holds N temporal
 * harmonics of M = (degree + 1)^2 SH coefficients, 0 <= N <= 3, 1 <= M <= 16:
 *     c_n(i)  = fp32(cos(2 pi n (time - t_i) / period)), argument and cosine in double
 *     shs[i]  = sum_n c_n(i) features_t[i][n]: one float32 fmaf chain in ascending n, started at features_t[i][0] (c_0 = 1)
 * shs [P][M][3].  N = 0 copies harmonic 0 bit for bit.  One launch; with N = 2 and M = 16 576 B read and 192 B written per Gaussian.
 *
 * gsr_harmonic_features_backward -- one launch:
 *     dL_dfeatures_t[i][n] = c_n(i) dL_dshs[i]                                                       (one float32 product)
 *     dL_dt[i]             = sum_n (2 pi n / period) sin(2 pi n (time - t_i) / period) <features_t[i][n], dL_dshs[i]>
 * the inner products in double, in a fixed order, with one owner per Gaussian.  Either output may be NULL and is then not written.
 * Accesses are 16 bytes wide where 3 M is a multiple of four and the pointers are 16-byte aligned, 4 bytes wide otherwise.
 *
 * No atomics anywhere: every output is bitwise reproducible from run to run.
 *
 * Refused with GSR_ERR_INVALID_ARGUMENT before any device work, with a message that starts with the function's name: a NULL required
 * pointer; P < 1; 6 P beyond 2^31 - 1 (the kernels index rows with 32 bits); a scaling modifier that is not finite or <= 0; a cutoff
 * outside [0, 1); a period that is not finite or <= 0; N outside 0..3; M outside 1..16; every output of a call NULL.
 * Profiling stages (gsr_profile_*): "slice4d_forward", "slice4d_backward", "harmonic_forward", "harmonic_backward".
 */
#ifndef GSR_SLICE4D_H_INCLUDED
#define GSR_SLICE4D_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_SLICE4D_THREADS 256     /* workgroup size of every kernel */
#define GSR_HARMONIC_MAX_N 3        /* temporal harmonics beside the constant one */
#define GSR_HARMONIC_MAX_M 16       /* SH coefficients per harmonic */

int gsr_slice4d_forward(int P, const float* xyz, const float* t, const float* scaling, const float* scaling_t, const float* rotation,
                        const float* rotation_r, const float* opacity, double time, double scaling_modifier, double cutoff,
                        float* means3D /* or NULL */, float* cov3D /* or NULL */, float* opacities /* or NULL */,
                        float* velocity /* or NULL */, void* stream);
int gsr_slice4d_backward(int P, const float* xyz, const float* t, const float* scaling, const float* scaling_t, const float* rotation,
                         const float* rotation_r, const float* opacity, double time, double scaling_modifier, double cutoff,
                         const float* dL_dmeans3D /* or NULL */, const float* dL_dcov3D /* or NULL */,
                         const float* dL_dopacities /* or NULL */, const float* dL_dvelocity /* or NULL */,
                         float* dL_dxyz /* or NULL */, float* dL_dt /* or NULL */, float* dL_dscaling /* or NULL */,
                         float* dL_dscaling_t /* or NULL */, float* dL_drotation /* or NULL */, float* dL_drotation_r /* or NULL */,
                         float* dL_dopacity /* or NULL */, void* stream);
int gsr_harmonic_features(int P, int N, int M, const float* features_t, const float* t, double time, double period, float* shs,
                          void* stream);
int gsr_harmonic_features_backward(int P, int N, int M, const float* features_t, const float* t, double time, double period,
                                   const float* dL_dshs, float* dL_dfeatures_t /* or NULL */, float* dL_dt /* or NULL */, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* GSR_SLICE4D_H_INCLUDED */
