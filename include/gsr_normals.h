/*
 * gsr_normals.h -- the two ends of the normal-consistency term of surface-reconstruction training on splats (2DGS, PGSR, RaDe-GS,
 * GOF, Gaussian surfels) in libgsr_hip.so (include/gsr.h): one normal per Gaussian, which the feature pass (gsr_features.h) blends
 * into a normal map with the colour pass's own weights, and the normals of a depth map's surface, alone or fused with the loss that
 * compares the two maps.  Entry points beside the core ABI of gsr.h, whose declarations and struct layouts they leave as they are;
 * none of them reads or writes the state of a forward.
 */
#ifndef GSR_NORMALS_H_INCLUDED
#define GSR_NORMALS_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
/*
 * ---- per-Gaussian normals ------------------------------------------------------------------------------------------------------
 * For Gaussian g with scales s = scales[g], quaternion q = rotations[g] = (w, x, y, z), mean m = means3D[g] and the view matrix V as
 * the rasterizer reads it (16 floats, element 4 * row + column of the transposed matrix, gsr.h):
 *   k    = the index of the smallest of s_0, s_1, s_2 under a strict <, so the first index wins an exact tie.  The scales are compared
 *          as given: log-scales (the leaf tensor) choose the same k as their exponentials.
 *   qn   = q / |q| (|q| = sqrt((w w + x x) + (y y + z z))); q = 0 gives a zero normal and a zero gradient
 *   n_w  = column k of the rotation matrix of qn,
 *            k = 0: (1 - 2 (y y + z z), 2 (x y + w z), 2 (x z - w y))
 *            k = 1: (2 (x y - w z), 1 - 2 (x x + z z), 2 (y z + w x))
 *            k = 2: (2 (x z + w y), 2 (y z - w x), 1 - 2 (x x + y y))
 *          the eigenvector of the covariance R S^2 R^T for the eigenvalue s_k^2
 *   t    = (V[0] m_x + V[4] m_y + V[8] m_z + V[12], V[1] m_x + V[5] m_y + V[9] m_z + V[13], V[2] m_x + V[6] m_y + V[10] m_z + V[14]),
 *          the view-space mean
 *   n_v  = the same expression of n_w without the translation V[12..14]
 *   sign = -1 if n_v . t > 0, else +1: every normal faces the camera (2DGS)
 *   out[g] = sign n_v for GSR_NORMALS_VIEW, sign n_w for GSR_NORMALS_WORLD
 * All P rows are written; nothing is culled.
 *
 * gsr_gaussian_normals_backward writes dL_drotations[g] = the gradient of sum_j dL_dout[g][j] out[g][j] with respect to q, with k
 * and sign held constant, through the normalisation (so each row is orthogonal to q).  scales, means3D and viewmatrix receive no
 * gradient.  All P rows are written.
 *
 * One Gaussian per lane, no atomics, results bitwise reproducible.  rotations and dL_drotations move as one 16-byte access per
 * Gaussian and must be 16-byte aligned.  Negative P, a space other than the two, and with P > 0 a NULL pointer or a misaligned
 * rotations / dL_drotations return GSR_ERR_INVALID_ARGUMENT before any device work, with a message that starts with the function's
 * name; P == 0 returns GSR_OK and launches nothing.  Profiling stages (gsr_profile_*): "gaussian_normals", "gaussian_normals_backward".
 */
#define GSR_NORMALS_VIEW 0
#define GSR_NORMALS_WORLD 1

int gsr_gaussian_normals(int P, const float* scales /* [P][3] */, const float* rotations /* [P][4] */, const float* means3D /* [P][3] */,
                         const float* viewmatrix /* [16] */, int space, float* out /* [P][3] */, void* stream);
int gsr_gaussian_normals_backward(int P, const float* scales, const float* rotations, const float* means3D, const float* viewmatrix,
                                  int space, const float* dL_dout /* [P][3] */, float* dL_drotations /* [P][4] */, void* stream);

/*
 * ---- depth normals -------------------------------------------------------------------------------------------------------------
 * Pixel (x, y) with view-space depth z stands for the point
 *   P(x, y) = (((2 x + 1) / W - 1) tanfovx z, ((2 y + 1) / H - 1) tanfovy z, z)
 * (the inverse of the rasterizer's pixel mapping for the centred principal point its settings assume).  For an interior pixel
 * (1 <= x <= W - 2, 1 <= y <= H - 2) whose four axis neighbours' depths are all finite and > 0,
 *   c   = (P(x, y + 1) - P(x, y - 1)) x (P(x + 1, y) - P(x - 1, y))
 *   n_d = c / max(|c|, 1e-12)
 * 2DGS's depth_to_normal in view space; a fronto-parallel plane gives (0, 0, -1), the facing of the per-Gaussian normals.  The
 * pixel's own depth does not enter.  n_d = 0 for border pixels and for every pixel with an invalid neighbour, and no gradient flows
 * through such a pixel.  The kernels evaluate c in the algebraically equal form
 *   c = (dy sv dh, dx sh dv, -(Y dx dv sh + X dy sv dh + dx dy sv sh))
 * with dv / sv the difference / sum of the lower and upper neighbours' depths, dh / sh those of the right and left ones, X, Y the
 * pixel's own factors of P and dx = 2 tanfovx / W, dy = 2 tanfovy / H: the differences of nearly equal products have cancelled.
 *
 * gsr_depth_normals writes out [3][H][W] in full.  gsr_depth_normals_backward writes dL_ddepth [H][W] in full: a pixel's depth
 * enters the normals of its four axis neighbours, whose contributions are gathered from a tile staged with its halo.
 *
 * ---- the normal-consistency loss ------------------------------------------------------------------------------------------------
 *   vals[0] = (1 / (H W)) sum_p (1 - a_p <N(p), n_d(p)>)          N = normal_map [3][H][W], a = alpha [H][W], a_p = 1 for alpha == NULL
 * 2DGS's normal_error.mean() with the depth normals multiplied by the detached alpha.  One call gives the value and, where asked for,
 *   dL_dnormal_map [3][H][W] = -a n_d / (H W)
 *   dL_ddepth      [H][W]    = the gradient through n_d
 * each written in full; alpha receives no gradient; a pixel without a depth normal contributes 1 to the sum and zeros to both
 * gradients, whatever normal_map holds there.  The sum is taken per workgroup and folded by one workgroup in a fixed order (double
 * precision); `scratch`: gsr_normals_scratch_bytes(W, H) bytes, contents irrelevant, free for reuse once the call's work on the
 * stream has finished.
 *
 * No atomics anywhere; all outputs are bitwise reproducible run to run.  Sizes that are not positive and NULL pointers (other than
 * the optional ones) return GSR_ERR_INVALID_ARGUMENT before any device work, with a message that starts with the function's name.
 * Profiling stages: "depth_normals", "depth_normals_backward", "normal_consistency_loss".
 */
size_t gsr_normals_scratch_bytes(int W, int H);   /* 0 for a size that is not positive */
int gsr_depth_normals(int W, int H, const float* depth /* [H][W] */, float tanfovx, float tanfovy, float* out /* [3][H][W] */, void* stream);
int gsr_depth_normals_backward(int W, int H, const float* depth, float tanfovx, float tanfovy, const float* dL_dout /* [3][H][W] */,
                               float* dL_ddepth /* [H][W] */, void* stream);
int gsr_normal_consistency_loss(int W, int H, const float* normal_map /* [3][H][W] */, const float* depth /* [H][W] */,
                                const float* alpha /* [H][W] or NULL */, float tanfovx, float tanfovy, float* vals /* [1] */,
                                float* dL_dnormal_map /* [3][H][W] or NULL */, float* dL_ddepth /* [H][W] or NULL */,
                                void* scratch, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* GSR_NORMALS_H_INCLUDED */
