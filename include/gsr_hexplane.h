/*
 * gsr_hexplane.h -- a plane-factorised feature grid over 3 or 4 input columns: the HexPlane / K-Planes encoding of the deformation-field
 * models (4DGaussians, K-Planes fields, tri-plane context models) in float32, whose second half is gsr_mlp.h.  A point is projected
 * onto every pair of axes, each projection interpolates bilinearly in a small 2-D feature plane, and the per-plane features are
 * multiplied together, at several resolutions.  Entry points beside the core ABI of gsr.h, whose declarations they leave as they are.
 * Nothing of size N x L x planes is ever written to memory, the forward saves nothing for the backward, and the table gradient is an
 * exact integer sum: its bits depend on neither the run, the order of the rows, nor the size of the scratch.
 *
 * Parameters.  D in {3, 4} input columns, L in 1 .. GSR_HEXPLANE_MAX_LEVELS levels, C channels, a multiple of 4 in 4 .. 64, one
 * resolution per level and axis res[l][a] in 2 .. 4096 (entries of res beyond L or D are ignored), N >= 0 rows.
 *
 * Planes.  P = D (D - 1) / 2 planes, the pairs (a, b), a < b, in lexicographic order: D = 3: (0,1) (0,2) (1,2); D = 4: (0,1) (0,2) (0,3)
 * (1,2) (1,3) (2,3).  A plane is a *time plane* when it holds axis 3.  The *flat index* of plane k of level l is l P + k.
 * table is one flat float32 array, level-major, then the planes in that order; a plane is [res_b][res_a][C], channels last, so the C
 * values of a node are contiguous.  gsr_hexplane_layout returns off[l P + k], in floats, and off[L P], the total.
 *
 * Forward, per row i.  This is grid_sample(bilinear, align_corners = true, padding_mode = border) per plane, product over the planes.
 *   void row   a row with a coordinate that is not finite (NaN, +-inf): every output of the row is +0, it adds nothing to dtable, and
 *              its dx row is +0.
 *   per axis a at level l, with u = x[i][a] and r = res[l][a]:
 *              s = (((double)u + 1.0) * 0.5) * (double)(r - 1), three double operations in this order (the unit is compiled
 *              uncontracted);  s < 0 becomes 0 and s > r - 1 becomes r - 1;  i0 = min((int)floor(s), r - 2);  frac = (float)(s - i0), an
 *              exact difference rounded once, so frac = 1 at the top node and no index leaves the plane.  The axis counts as *clamped*
 *              when u <= -1 or u >= 1 (torch's rule for the gradient of border padding).
 *   weights    along an axis a corner has the float32 weight 1.0f - frac (node i0) or frac (node i0 + 1); the corner's weight is the
 *              float32 product w = w_b * w_a.
 *   corners    visited in the order (b0,a0), (b0,a1), (b1,a0), (b1,a1); the node (ib, ia) of plane (a, b) is element
 *              (ib * res_a + ia) * C + c of the plane.
 *   plane      p_k[c] = the float32 chain acc = fmaf(w, v, acc) over the corners in that order from +0.
 *   level      z_l[c] = ((p_0 * p_1) * p_2) ... in float32, planes ascending.
 *   output     concat != 0: y is N x (L C), y[i][l C + c] = z_l[c];  concat == 0: y is N x C, y[i][c] = the float32 sum of z_l[c] over the
 *              levels ascending from +0.  dy has y's shape; below dy_l[c] is dy[i][l C + c] or, without concat, dy[i][c] for every l.
 *
 * Backward, table.  dtable[node of plane k of level l][c] = sum over the rows and the (at most four) corners that address the node of
 * w g_k, where g_k = dy_l[c] prod_{j != k} p_j[c], defined so that the order of the additions cannot matter:
 *   g_k    formed in double from the float32 p_j (computed again, nothing is saved): g = (double)dy_l[c], then g = g * (double)p_j for
 *          j != k ascending, one double product each.
 *   m      the largest |dy| of the call, over every row (void ones included) and every column of dy, as the maximum of the bit patterns
 *          with the sign cleared;  M_{l,j} likewise the largest |v| of plane j of level l, from one pass over the table.  A NaN or an
 *          infinity anywhere in dy or in table makes every element of dtable NaN (decided on the device, nothing is read back).
 *   Bnd    = m prod_{j != k} M_{l,j} in double: Bnd = (double)m, then Bnd = Bnd * (double)M_{l,j} for j != k ascending; a product of at
 *          most six float32, so it is exact up to rounding, never subnormal and never overflows.  Bnd = 0 makes plane k of level l +0
 *          throughout.  Otherwise
 *   e      = ilogb(Bnd) + 2,  B = the smallest integer with 2^B >= 4 N,  q = 62 - B - e (in -740 .. 952: 2^q is a normal double).
 *   t      = llrint(ldexp((double)w * g_k, q)): one double product, an exact scaling, rounding to nearest even
 *   S      = sum of t in int64;  dtable = (float)ldexp((double)S, -q), both conversions to nearest even.
 * Why nothing overflows.  0 <= w <= 1 (a float32 product of two float32 in [0, 1]).  p_j is a float32 chain over four corners whose float32
 * weights sum to at most 1 + 2^-22, and each of its four fmaf steps rounds once, so |p_j| <= M_{l,j} (1 + 2^-21); over at most five
 * planes and the double roundings of g_k and Bnd, |w g_k| <= Bnd (1 + 2^-18) < 2^(ilogb(Bnd) + 1) (1 + 2^-18) < 2^e: this is what the spare
 * binade of e pays for.  So |t| <= 2^(q + e) <= 2^(62 - B).  The corners of a row are four different nodes (i0 + 1 <= r - 1 differs from i0),
 * so a node receives at most N <= 2^(B - 2) terms per channel and |S| <= 2^60 < 2^62.  Integer addition is associative, so S has the same
 * value however the terms meet: 64-bit integer atomics in global memory, in LDS, in any order, in any number of passes.
 * Error: |dtable - exact sum of w g_k| <= n_e 2^-(q+1) + one float32 rounding of the result (plus one double rounding per product of
 * g_k and w g_k, 2^-53 relative each, and one double rounding of S when |S| >= 2^53, below the float32 one by 2^-29); n_e is the number of
 * terms of the node, and 2^-(q+1) lies 61 - B bits below Bnd's binade.
 *
 * Backward, x (optional).  One owner per row, double accumulators, rounded once to float32: for levels ascending, channels ascending
 * and planes k = (a, b) ascending, with g_k as above,
 *   acc[a] += g_k * ((double)(res_a - 1) * 0.5) * da,   da = (1 - fb) (v01 - v00) + fb (v11 - v10)
 *   acc[b] += g_k * ((double)(res_b - 1) * 0.5) * db,   db = (1 - fa) (v10 - v00) + fa (v11 - v01)
 * where v00, v01, v10, v11 are the corner values in the corner order and fa, fb, 1 - fa, 1 - fb the float32 axis weights, everything
 * converted to double and every operation a double one in the order written.  A clamped axis gets exactly +0 and so does a void row.
 * All D columns get a gradient, time included.  The row's bits do not depend on where in x it stands.
 *
 * Paths of the table backward (gsr_hexplane_level_path, per level and plane): GSR_HEXPLANE_PATH_LDS when the plane's sums for a slice
 * of four channels, res_a res_b 4 8 bytes, fit GSR_HEXPLANE_LDS_BYTES -- up to 64 x 64 nodes: a workgroup owns one (plane, channel
 * slice, row chunk), sums in LDS and flushes its non-zero sums once --, and GSR_HEXPLANE_PATH_DIRECT otherwise (global 64-bit integer
 * atomics, the lanes laid along the channels).  Both form the same S.
 *
 * Regulariser (gsr_hexplane_regularizer).  For a plane v[res_b][res_a][C], with first differences D_b v = v[b+1] - v[b] etc.:
 *   tv     = 2 (sum (D_b v)^2 / ((res_b - 1) res_a C) + sum (D_a v)^2 / (res_b (res_a - 1) C))
 *   smooth = sum (D_b D_b v)^2 / ((res_b - 2) res_a C), the second difference along the slow axis (the time axis of every time
 *            plane); 0 for res_b < 3
 *   l1     = sum |1 - v| / (res_b res_a C)
 * value = w_tv_space sum tv + w_smooth_space sum smooth over the planes without axis 3 of every level
 *       + w_tv_time sum tv + w_smooth_time sum smooth + w_l1_time sum l1 over the time planes of every level,
 * every difference, square and sum in double (the sum over the table in a fixed order that depends on the shape only), rounded once;
 * dtable, if wanted, is its gradient, every element a double sum of at most nine terms rounded once (the derivative of |1 - v| at
 * v = 1 is 0).  One pass over the table and a fold, no atomics: the same bits on every run.  N and the strides of desc are not read.
 *
 * Strides are counted in floats: element (row, c) of x at [row * x_stride + c]; likewise y and dy (L C columns, or C without concat; a
 * column slice of a wider matrix is read in place) and dx (D columns).
 *
 * gsr_hexplane_scratch_bytes  *min_bytes: what a backward needs at the least (the small words and the sums of the largest plane);
 *                   *full_bytes: what lets it run every plane in one pass.  Either pointer may be NULL.  Independent of N.
 * gsr_hexplane_forward   y from x and table.  No scratch.
 * gsr_hexplane_backward  dx (N x D) and dtable (as table), each may be NULL: what is NULL is neither formed nor written, and the bits
 *                   of the other do not depend on it.  scratch is read only for dtable: scratch_bytes >= min, 16-byte aligned, contents
 *                   irrelevant, free for reuse once the call's work on the stream has finished; consecutive planes are processed in as
 *                   many passes as scratch_bytes requires, and the result does not depend on it.  N == 0 writes +0 to dtable.
 * gsr_hexplane_regularizer   *value (one float on the device) and dtable (or NULL); scratch of at least GSR_HEXPLANE_REG_SCRATCH_BYTES,
 *                   16-byte aligned.
 *
 * Refused with GSR_ERR_INVALID_ARGUMENT (-1) before any device work, with a gsr_last_error() text that starts with the function's
 * name: a NULL desc; N < 0; D, L, C or a resolution outside its range; a stride smaller than its column count; a NULL pointer where
 * N > 0 (x, table, y or dy); for a wanted dtable a NULL scratch, one that is not 16-byte aligned or one below the minimum; for the
 * regulariser a NULL table or value and the same three of its scratch.  Every element index is formed in 64 bits.
 * Profiling stages (gsr_profile_*): "hexplane_forward", "hexplane_backward", "hexplane_regularizer"; recorded only when asked for by
 * name (gsr_profile_begin_only), the two table-gradient kernels alone: "hexplane_backward_lds", "hexplane_backward_direct", one entry
 * per pass.
 */
#ifndef GSR_HEXPLANE_H_INCLUDED
#define GSR_HEXPLANE_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_HEXPLANE_MAX_LEVELS 8
#define GSR_HEXPLANE_MAX_PLANES 6
#define GSR_HEXPLANE_MAX_RES 4096
#define GSR_HEXPLANE_LDS_BYTES (128 * 1024)
#define GSR_HEXPLANE_REG_SCRATCH_BYTES 65536

#define GSR_HEXPLANE_PATH_DIRECT 0
#define GSR_HEXPLANE_PATH_LDS 1

typedef struct gsr_hexplane_desc {
	int N;                                    /* rows */
	int D, L, C;                              /* input columns, levels, channels */
	int concat;                               /* != 0: the levels side by side; 0: summed */
	int res[GSR_HEXPLANE_MAX_LEVELS][4];      /* res[l][a] */
	long long x_stride, y_stride, dy_stride, dx_stride;   /* in floats; dy_stride and dx_stride are read by the backward only */
} gsr_hexplane_desc;

/* host only: offsets[L P + 1] in floats */
int gsr_hexplane_layout(const gsr_hexplane_desc* desc, long long* offsets);
int gsr_hexplane_level_path(const gsr_hexplane_desc* desc, int level, int plane);   /* GSR_HEXPLANE_PATH_*; -1 outside the limits */
int gsr_hexplane_scratch_bytes(const gsr_hexplane_desc* desc, size_t* min_bytes, size_t* full_bytes);
int gsr_hexplane_forward(const gsr_hexplane_desc* desc, const float* x, const float* table, float* y, void* stream);
int gsr_hexplane_backward(const gsr_hexplane_desc* desc, const float* x, const float* table, const float* dy, float* dx /* or NULL */,
                          float* dtable /* or NULL */, void* scratch, size_t scratch_bytes, void* stream);
int gsr_hexplane_regularizer(const gsr_hexplane_desc* desc, const float* table, float w_tv_space, float w_tv_time, float w_smooth_space,
                             float w_smooth_time, float w_l1_time, float* value, float* dtable /* or NULL */, void* scratch,
                             size_t scratch_bytes, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* GSR_HEXPLANE_H_INCLUDED */
