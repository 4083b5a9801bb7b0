/*
 * gsr_hashgrid.h -- a multiresolution (hashed) feature grid over 2, 3 or 4 input columns, tiny-cuda-nn's GridEncoding with linear
 * interpolation in float32: the first half of the hash-grid + small-MLP fields of Compact-3DGS, HAC, Grid4D and the hash-encoded
 * deformation fields, whose second half is gsr_mlp.h.  Entry points beside the core ABI of gsr.h, whose declarations they leave as
 * they are.  Nothing of size N x L x 2^D is ever written to memory, the forward saves nothing for the backward, and the table
 * gradient is an exact integer sum: its bits depend on neither the run, the order of the rows, nor the size of the scratch.
 *
 * Parameters.  D in {2, 3, 4} input columns, L in 1 .. GSR_HASHGRID_MAX_LEVELS levels, F in {1, 2, 4, 8} features per entry,
 * base_resolution >= 1, per_level_scale >= 1 (a float), log2_hashmap_size in 1 .. 24, N >= 0 rows.
 *
 * Level table (host, float32 operations, one rounding each -- exp2f and log2f stand for the correctly rounded functions, formed as the
 * double function rounded to float32; gsr_hashgrid_layout and gsr_hashgrid_level_scale return it):
 *   scale_l = exp2f((float)l * log2f(per_level_scale)) * (float)base_resolution - 1.0f
 *   res_l   = (uint32)ceilf(scale_l) + 1                      (a desc whose finest res_l exceeds 2^30 is refused)
 *   size_l  = min(round_up(res_l^D, 8), 2^log2_hashmap_size)  (the power formed in 64 bits, saturating)
 *   off_0 = 0, off_{l+1} = off_l + size_l;  the level is *dense* when res_l^D <= size_l, otherwise *hashed*.
 * table is [off_L][F] float32: level-major, the F features of an entry contiguous.  This is tiny-cuda-nn's layout, written from its
 * published source; that a table trained there loads here with the same meaning is intended and has not been verified.
 *
 * Forward, per row i and level l:
 *   void row   a row with a coordinate that is not finite (NaN, +-inf): every output of the row is +0, it adds nothing to dtable, and
 *              its dx row is +0.
 *   clamp      xc_a = x_a < 0 ? 0 : x_a > 1 ? 1 : x_a;  the axis counts as *clamped* when x_a < 0 or x_a > 1.
 *   position   p_a = (double)xc_a * (double)scale_l + 0.5, the product and the sum two double operations (the unit is compiled
 *              uncontracted);  cell_a = floor(p_a);  c_a = (uint32)cell_a;  frac_a = (float)(p_a - cell_a): an exact difference, rounded once.
 *   weights    along axis a a corner has the float32 weight frac_a (its +1 side) or 1.0f - frac_a; the corner's weight w is the
 *              float32 product of its axis weights taken axis 0 first: ((w_0 w_1) w_2) w_3.
 *   corners    visited in ascending corner code k = 0 .. 2^D - 1; bit a of k is the +1 along axis a, g_a = c_a + bit_a(k).
 *   index      dense:  sum_a g_a * res_l^a in uint32 (res_l^a a uint32 product, wrapping);
 *              hashed: g_0 * 1 ^ g_1 * 2654435761 ^ g_2 * 805459861 ^ g_3 * 3674653429 in uint32 (wrapping);
 *              either is then taken mod size_l, always: no input whatsoever addresses outside its level.  (This keeps tiny-cuda-nn's
 *              quirk that the +1 corner of the top cell of a dense level aliases into the next row of the level.)
 *   output     y[i][l F + f] = the float32 chain acc = fmaf(w_k, table[off_l + idx_k][f], acc) over the corners in that order from +0.
 *
 * Backward, table.  dtable[e][f] = sum over (row, level, corner) with off_l + idx = e of w dy[i][l F + f], defined so that the order
 * of the additions cannot matter:
 *   m = the largest |dy[i][c]| of the call, over every row (void ones included) and every column c < L F, as the maximum of the bit
 *       patterns with the sign cleared.  A NaN or an infinity anywhere in dy makes every element of dtable NaN (decided on the device,
 *       nothing is read back); m = 0 makes every element +0.  Otherwise
 *   e = ilogb(m) + 1,  B = the smallest integer with 2^B >= N 2^D,  q = 62 - B - e;
 *   t = llrint(ldexp((double)w * (double)dy, q))     the product of two float32 is exact in double; llrint rounds to nearest even
 *   S[e][f] = sum t in int64: |t| <= 2^(62 - B) and an entry has at most N 2^D <= 2^B terms, so |S| <= 2^62 and nothing overflows
 *   dtable[e][f] = (float)ldexp((double)S, -q), both conversions to nearest even.
 * Integer addition is associative, so S has the same value however the terms meet: 64-bit integer atomics in global memory, in LDS,
 * in any order, in any number of passes.  Error: |dtable - exact| <= n_e 2^-(q+1) + one float32 rounding of the result (plus one
 * double rounding of S when |S| >= 2^53, below the float32 one by 2^-29), n_e the number of terms of the entry; 2^-(q+1) lies at
 * least 61 - B bits below m's binade: 39 bits below it at 2^20 rows and D = 3, against 24 for a float32 sum.
 *
 * Backward, x (optional).  With u_a = the axis weight of the corner along a and s_a = +1 on the +1 side, -1 on the other,
 *   dx[i][a] = the double sum, rounded once to float32, over levels ascending, corners ascending, features ascending of
 *              (double)scale_l * s_a * (prod_{b != a} (double)u_b, b ascending) * (double)dy[i][l F + f] * (double)table[..][f]
 * (the corner's inner sum over f is formed first, then scaled).  A clamped axis gets exactly +0, and so does a void row.  One owner
 * per row, no atomics: the row's bits do not depend on where in x it stands.
 *
 * Levels take one of two paths in the table backward (gsr_hashgrid_level_path): GSR_HASHGRID_PATH_LDS for a dense level whose sums,
 * size_l F 8 bytes, fit GSR_HASHGRID_LDS_BYTES (workgroups sum their rows in LDS and flush once, contiguously), and
 * GSR_HASHGRID_PATH_DIRECT otherwise (one global 64-bit integer atomic per term).  Both form the same S.
 *
 * Strides are counted in floats: element (row, c) of x at [row * x_stride + c]; likewise y (L F columns), dy (L F columns: a column
 * slice of a wider matrix is read in place) and dx (D columns).
 *
 * gsr_hashgrid_scratch_bytes  *min_bytes: what a backward needs at the least (the small words and the sums of the largest level);
 *                   *full_bytes: what lets it run every level in one pass.  Either pointer may be NULL.  Independent of N.
 * gsr_hashgrid_forward   y from x and table.  No scratch.
 * gsr_hashgrid_backward  dx (N x D) and dtable (as table), each may be NULL: what is NULL is neither formed nor written, and the bits
 *                   of the other do not depend on it.  scratch is read only for dtable: scratch_bytes >= min, 16-byte aligned, contents
 *                   irrelevant, free for reuse once the call's work on the stream has finished; the levels are processed in as many
 *                   passes as scratch_bytes requires, and the result does not depend on it.  N == 0 writes +0 to dtable.
 *
 * Refused with GSR_ERR_INVALID_ARGUMENT (-1) before any device work, with a gsr_last_error() text that starts with the function's
 * name: a NULL desc; N < 0 (an int: N < 2^31 holds by type); D, L, F, base_resolution, per_level_scale or log2_hashmap_size outside
 * its range; a finest resolution above 2^30; a stride smaller than its column count; a NULL pointer where N > 0 (x, table, y or dy);
 * for a wanted dtable a NULL scratch, one that is not 16-byte aligned or one below the minimum.  With N < 2^31 and L F <= 256 every
 * element index fits 64 bits and every launch fits the grid limits, so no count needs a refusal of its own.
 * Profiling stages (gsr_profile_*): "hashgrid_forward", "hashgrid_backward".
 */
#ifndef GSR_HASHGRID_H_INCLUDED
#define GSR_HASHGRID_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_HASHGRID_MAX_LEVELS 32
#define GSR_HASHGRID_MAX_LOG2_SIZE 24
#define GSR_HASHGRID_LDS_BYTES (128 * 1024)

#define GSR_HASHGRID_PATH_DIRECT 0
#define GSR_HASHGRID_PATH_LDS 1

typedef struct gsr_hashgrid_desc {
	int N;                                    /* rows */
	int D, L, F;                              /* input columns, levels, features per entry */
	int base_resolution;
	float per_level_scale;
	int log2_hashmap_size;
	long long x_stride, y_stride, dy_stride, dx_stride;   /* in floats; dy_stride and dx_stride are read by the backward only */
} gsr_hashgrid_desc;

/* host only: offsets[L + 1] in entries, resolutions[L], hashed[L] (1 = hashed, 0 = dense); any of the three may be NULL */
int gsr_hashgrid_layout(const gsr_hashgrid_desc* desc, long long* offsets, int* resolutions, int* hashed);
float gsr_hashgrid_level_scale(const gsr_hashgrid_desc* desc, int level);   /* scale_l; NaN for a desc or level outside the limits */
int gsr_hashgrid_level_path(const gsr_hashgrid_desc* desc, int level);      /* GSR_HASHGRID_PATH_*; -1 for a desc or level outside the limits */
int gsr_hashgrid_scratch_bytes(const gsr_hashgrid_desc* desc, size_t* min_bytes, size_t* full_bytes);
int gsr_hashgrid_forward(const gsr_hashgrid_desc* desc, const float* x, const float* table, float* y, void* stream);
int gsr_hashgrid_backward(const gsr_hashgrid_desc* desc, const float* x, const float* table, const float* dy, float* dx /* or NULL */,
                          float* dtable /* or NULL */, void* scratch, size_t scratch_bytes, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* GSR_HASHGRID_H_INCLUDED */
