/*
 * gsr_mlp.h -- a fully fused small MLP on the fp32-input matrix cores, with an optional frequency encoding of its input: the anchor
 * decoders of Scaffold-GS, the deformation fields of Deformable-3DGS, per-pixel decoders of rendered feature maps.  Entry points
 * beside the core ABI of gsr.h, whose declarations they leave as they are.  Nothing of size N x hidden is ever written to memory;
 * the forward saves nothing for the backward, which recomputes it.
 *
 * The rule.  A network is M linear maps, 1 <= M <= GSR_MLP_MAX_LAYERS, with widths d_0 .. d_M, each in 1 .. GSR_MLP_MAX_WIDTH.
 * weights[l-1] = W_l [d_l][d_{l-1}] float32 row-major (torch.nn.Linear's layout), biases[l-1] = b_l [d_l] or NULL = +0; N >= 0 rows.
 *
 *   encoding   L octaves, 0 <= L <= GSR_MLP_MAX_OCTAVES, over D raw columns: d_0 = D (1 + 2 L), and the encoded row is
 *              (x, sin(2^0 x), cos(2^0 x), .., sin(2^{L-1} x), cos(2^{L-1} x)), each block D wide.  2^j x is an exact float32 product;
 *              sin and cos are taken in double of it and rounded once.  The encoded row exists on chip only.
 *   linear     z_l[o] = the chain acc = fmaf(W_l[o][k], a_{l-1}[k], acc) for k = 0 .. d_{l-1}-1 ascending, started at b_l[o] (+0
 *              without a bias): what v_mfma_f32_32x32x2_f32 computes with the bias as its C input.  (Its k dimension is padded with
 *              zero weights against zero activations; fmaf(0, 0, acc) has acc's value, and a z of -0 may come out as +0.)
 *   hidden     GSR_MLP_RELU: a = (z <= 0) ? +0 : z, so NaN propagates and -0 becomes +0; the backward mask is z > 0.
 *              GSR_MLP_NONE: a = z, mask 1.
 *   output     y = z_M (GSR_MLP_NONE), 1 / (1 + exp(-z_M)) (GSR_MLP_SIGMOID) or tanh(z_M) (GSR_MLP_TANH), evaluated in double on
 *              the float32 z_M and rounded once.
 *   backward   dz_M = dy act'(z_M), a double product rounded once, with act' formed in double from z_M: s(z) s(-z) for the sigmoid
 *              s, 1 - tanh(z)^2; dy itself for GSR_MLP_NONE.
 *              da_{l-1}[k] = the chain acc = fmaf(W_l[o][k], dz_l[o], acc) for o = 0 .. d_l-1 ascending from +0;
 *              dz_{l-1} = mask ? da_{l-1} : +0.
 *              Through the encoding, in double, the terms added in ascending j and the result rounded once:
 *              dx = g_x + sum_j 2^j (cos(2^j x) g_sin,j - sin(2^j x) g_cos,j), g = da_0.
 *              dW_l[o][k] = sum_rows dz_l[row][o] a_{l-1}[row][k],  db_l[o] = sum_rows dz_l[row][o]: float32 sums in this order.
 *              The rows are cut into tiles of R rows, R = gsr_mlp_tile_rows(), a function of the widths alone.  There are
 *              G = min(ceil(N / R), max_workgroups) workgroups (max_workgroups 0 = GSR_MLP_DEFAULT_WORKGROUPS), and workgroup g
 *              owns the tiles g, g + G, ..  Its partial of dW is the chain acc = fmaf(dz[row][o], a[row][k], acc) from +0 over its
 *              rows in ascending row order (the MFMA again, the row as its k), its partial of db the chain acc = acc + dz[row][o].
 *              The result is ((partial_0 + partial_1) + partial_2) .. in ascending g, formed by one owner per element.  No atomics
 *              of any kind: every output has the same bits every run, whatever the device.
 *
 * Layouts.  x and y are each GSR_MLP_ROWS, element (row, c) at [row * stride + c], or GSR_MLP_PLANES, at [c * stride + row]; the
 * strides are counted in floats.  dy has y's layout and dy_stride, dx x's layout and dx_stride.  A rendered feature_map (K, H, W)
 * is GSR_MLP_PLANES with stride H W.
 *
 * gsr_mlp_forward   y from x.  scratch: gsr_mlp_scratch_bytes(desc) bytes, 16-byte aligned, contents irrelevant, free for reuse once
 *                   the call's work on the stream has finished.
 * gsr_mlp_backward  dx (N x D), dW[l-1] as W_l, db[l-1] as b_l.  Each of dx, dW, db may be NULL, and so may single entries of dW
 *                   and db: what is NULL is neither formed nor written, and the bits of the others do not depend on it.
 *                   N == 0 writes zeros to the wanted dW and db and nothing else.
 *
 * Refused with GSR_ERR_INVALID_ARGUMENT (-1) before any device work, with a gsr_last_error() text that starts with the function's
 * name: a NULL desc; N < 0; M, a width, D or L outside its range; d_0 != D (1 + 2 L); an unknown activation or layout; a stride
 * smaller than the layout needs (rows: the column count, planes: N); a NULL pointer where N > 0 (x, weights, any weights[l], y or
 * dy, scratch); scratch that is not 16-byte aligned; a negative max_workgroups.
 * Profiling stages (gsr_profile_*): "mlp_forward", "mlp_backward".
 */
#ifndef GSR_MLP_H_INCLUDED
#define GSR_MLP_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_MLP_MAX_LAYERS 5
#define GSR_MLP_MAX_WIDTH 128
#define GSR_MLP_MAX_OCTAVES 10
#define GSR_MLP_DEFAULT_WORKGROUPS 256

#define GSR_MLP_NONE 0
#define GSR_MLP_RELU 1
#define GSR_MLP_SIGMOID 2
#define GSR_MLP_TANH 3

#define GSR_MLP_ROWS 0
#define GSR_MLP_PLANES 1

typedef struct gsr_mlp_desc {
	int N;                                    /* rows */
	int M;                                    /* linear maps */
	int widths[GSR_MLP_MAX_LAYERS + 1];       /* d_0 .. d_M */
	int D, L;                                 /* raw input columns and octaves; d_0 = D (1 + 2 L) */
	int hidden_activation;                    /* GSR_MLP_NONE or GSR_MLP_RELU */
	int output_activation;                    /* GSR_MLP_NONE, GSR_MLP_SIGMOID or GSR_MLP_TANH */
	int x_layout, y_layout;                   /* GSR_MLP_ROWS or GSR_MLP_PLANES */
	long long x_stride, y_stride, dy_stride, dx_stride;   /* in floats; dy_stride and dx_stride are read by the backward only */
	int max_workgroups;                       /* of the backward; 0 = GSR_MLP_DEFAULT_WORKGROUPS */
} gsr_mlp_desc;

int gsr_mlp_tile_rows(const gsr_mlp_desc* desc);        /* R of the rule; 0 for a desc outside the limits */
size_t gsr_mlp_scratch_bytes(const gsr_mlp_desc* desc); /* 0 for a desc outside the limits */
int gsr_mlp_forward(const gsr_mlp_desc* desc, const float* x, const float* const* weights, const float* const* biases /* or NULL */,
                    float* y, void* scratch, void* stream);
int gsr_mlp_backward(const gsr_mlp_desc* desc, const float* x, const float* const* weights, const float* const* biases /* or NULL */,
                     const float* dy, float* dx /* or NULL */, float* const* dW /* or NULL */, float* const* db /* or NULL */,
                     void* scratch, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* GSR_MLP_H_INCLUDED */
