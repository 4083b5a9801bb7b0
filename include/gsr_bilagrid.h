/*
 * gsr_bilagrid.h -- the per-image bilateral grid of affine colour transforms ("Bilateral Guided Radiance Field Processing"; gsplat's
 * lib_bilagrid `slice` and `total_variation_loss`): the spatially varying form of the 3x4 exposure of gsr_loss_ext.h.  Entry points
 * beside the core ABI of gsr.h, whose declarations they leave as they are.
 *
 * All arrays are float32 on the device.  grid [12][L][GH][GW] is ONE image's grid: channel 4c + k holds entry A[c][k] of a 3x4
 * matrix, L is the guidance (luma) axis, GH and GW the spatial axes, each of the three >= 2.  img [3][H][W], H, W >= 1.  For the
 * pixel (y, x) with colour (r, g, b):
 *
 *   gx   = (x + 0.5) / W * (GW - 1),   gy = (y + 0.5) / H * (GH - 1)
 *   luma = 0.299 r + 0.587 g + 0.114 b,   gz = clamp(luma * (L - 1), 0, L - 1)
 *   A[c][k] = trilinear interpolation of channel 4c + k at (gz, gy, gx): cell index floor(), capped at size - 2; weights 1 - t, t
 *   out_c   = A[c][0] r + A[c][1] g + A[c][2] b + A[c][3]                       (out [3][H][W])
 *
 * i.e. grid_sample(bilinear, align_corners, border padding) at pixel centres followed by the affine product.
 *
 * Gradients, with G = dL_dout [3][H][W] and v = (r, g, b, 1), each written in full where its pointer is not NULL:
 *   dL_dgrid[4c + k][node] = sum over pixels of w(node, pixel) G_c v_k, w the product of the three hat weights; a node that no pixel
 *                            reaches gets +0.0
 *   dL_dimg[k] = sum_c A[c][k] G_c  +  lw_k (L - 1) sum_c G_c sum_k' (A_z1[c][k'] - A_z0[c][k']) v_k'
 *                lw = (0.299, 0.587, 0.114); A_z0, A_z1 the bilinear-in-xy values on the two luma levels of the pixel's cell; the
 *                second (guidance) part is exactly zero where luma (L - 1) <= 0 or >= L - 1
 *
 * Total variation of grids [N][12][L][GH][GW]:
 *   tv = (1 / N) sum over the axes a in {L, GH, GW} of  sum (g[i + 1 along a] - g[i])^2 / count_a
 * count_a the number of such differences in ONE image's grid (12 (L - 1) GH GW for the luma axis).  gsr_bilagrid_tv writes the value
 * to val[0] and, where dL_dgrids is not NULL, d tv / d grids (the two-sided stencil) in the same pass.
 *
 * No atomics anywhere.  dL_dgrid is a gather: one workgroup per spatial node and group of four luma levels walks the pixels of that
 * node's support in a fixed order and reduces them in a fixed order (lanes, then waves); where the grid has too few nodes to fill
 * the device the support is cut into row segments whose partial sums lie in `scratch` and are added in segment order in double
 * precision.  The tv value is a per-workgroup sum in a fixed order and one fold in double precision.  Every output is bitwise
 * reproducible run to run.  `scratch`: gsr_bilagrid_scratch_bytes(...) resp. gsr_bilagrid_tv_scratch_bytes(...) bytes, contents
 * irrelevant, free for reuse once the call's work on the stream has finished.
 *
 * gsr_bilagrid_slice needs grid, img and out.  gsr_bilagrid_slice_backward needs grid, img, dL_dout, at least one of dL_dgrid and
 * dL_dimg, and scratch with dL_dgrid; a gradient pointer left NULL is not computed.  The fields a call does not name are ignored.
 *
 * Refused with GSR_ERR_INVALID_ARGUMENT before any device work, with a message that starts with the function's name: NULL args;
 * H or W < 1; L, GH or GW < 2; N < 1; a NULL required pointer; 3 H W, 12 L GH GW or N 12 L GH GW above 2^31 - 1 (the kernels index
 * with 32 bits); more than 2^24 - 1 workgroups in one launch.
 * Profiling stages (gsr_profile_*): "bilagrid_slice", "bilagrid_backward", "bilagrid_tv".
 */
#ifndef GSR_BILAGRID_H_INCLUDED
#define GSR_BILAGRID_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct gsr_bilagrid_args {
    int H, W, L, GH, GW;
    const float *grid, *img;          /* [12][L][GH][GW], [3][H][W] */
    float *out;                       /* [3][H][W]: gsr_bilagrid_slice */
    const float *dL_dout;             /* [3][H][W]: gsr_bilagrid_slice_backward */
    float *dL_dgrid, *dL_dimg;        /* [12][L][GH][GW], [3][H][W]; each or NULL */
    void *scratch, *stream;
} gsr_bilagrid_args;

size_t gsr_bilagrid_scratch_bytes(int H, int W, int L, int GH, int GW);   /* 0 for a size that is not valid */
int gsr_bilagrid_slice(const gsr_bilagrid_args* args);
int gsr_bilagrid_slice_backward(const gsr_bilagrid_args* args);

size_t gsr_bilagrid_tv_scratch_bytes(int N, int L, int GH, int GW);       /* 0 for a size that is not valid */
int gsr_bilagrid_tv(int N, int L, int GH, int GW, const float* grids, float* val, float* dL_dgrids /* or NULL */, void* scratch,
                    void* stream);
#ifdef __cplusplus
}
#endif
#endif /* GSR_BILAGRID_H_INCLUDED */
