// gsr_rect_trim.h -- which tiles of its rectangle a Gaussian can reach at all, and how the binning is told.
//
// The reference bins a Gaussian into every tile of the square of 3 sigma (radius rounded up) around its centre
// (getRect, auxiliary.h:42-58; duplicateWithKeys, rasterizer_impl.cu:78-126), and the blend loops then find, pixel by pixel, that
// most of those tiles hold no pixel with alpha >= 1 / 255 (forward.cu:449-456, backward.cu:527-534): the splat is an ellipse, its
// opacity lowers the threshold, and the square is rounded up to tiles.  At 1 M Gaussians / 1080p 9.2 M instances are binned and 53 %
// of them can contribute somewhere in their tile.  An instance that contributes to no pixel of its tile changes nothing: not the
// pixels' T or colour, not n_contrib's meaning for the backward (the position of the last contributor in the list the backward walks
// -- the same list), no gradient.  So the column-pair binning (tilebin.hip) leaves out tiles that the ellipse
//     conic_a dx^2 + 2 conic_b dx dy + conic_c dy^2 <= 2 ln(255 opacity)            (alpha >= 1 / 255  <=>  power >= -ln(255 opacity))
// provably misses, per tile COLUMN of the rectangle: up to three tile rows off the top and up to three off the bottom of every
// column (two bits each: a nibble per column, eight columns in one word), empty columns off the left and right edge.  A rectangle
// wider than eight tiles shares a nibble among 2, 4, ... 32 neighbouring columns, one taller than 16 tiles counts the rows in units
// of 2, 4, ... 16: coarser, never wrong.  What is kept is a superset of what can contribute IN THE KERNELS' ARITHMETIC: the bound is
// taken over the column's whole strip of pixel centres, the conic's determinant enters by a lower bound of its fp32 value, and the
// threshold grows with the magnitude of the terms that cancel in the kernels' fp32 `power` (both derived in gsr_rect_trim below; a
// constant margin covers an ordinary splat and loses tiles of a needle 1000 px long whose centre lies far off the pixels it covers),
// so every output -- image, radii, gradients -- has the same bits with and without it (GSR_DEBUG_NO_TRIM; tests/test_trim_gpu.py,
// tests/test_trim_needles_gpu.py, tests/test_trim_needles_cpu.py, tools/trim_stress.py, tools/determinism_stress.py), and the slots of
// the left-out instances are exactly slots the backward never marks valid.  num_rendered, tiles_touched and the gradient slots keep
// the reference's numbering over the WHOLE rectangle; point_list and the tile ranges are the reference's with the left-out instances
// removed (the reference's own, bit for bit, with GSR_DEBUG_NO_TRIM and on the tile-sort path).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the rectangle in one word (tile coordinates < 256, sizes 1 .. 256); no tiles: GSR_RECT_NONE
#define GSR_RECT_NONE 0xFFFFFFFFu
__host__ __device__ __forceinline__ uint32_t gsr_rect_pack(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h)
{
	return (w == 0u || h == 0u) ? GSR_RECT_NONE : (x0 | (y0 << 8) | ((w - 1u) << 16) | ((h - 1u) << 24));
}
__host__ __device__ __forceinline__ void gsr_rect_unpack(uint32_t r, uint32_t& x0, uint32_t& y0, uint32_t& w, uint32_t& h)
{
	if (r == GSR_RECT_NONE) { x0 = y0 = w = h = 0u; return; }
	x0 = r & 0xffu; y0 = (r >> 8) & 0xffu; w = ((r >> 16) & 0xffu) + 1u; h = (r >> 24) + 1u;
}

#define GSR_TRIM_GROUPS 8        // nibbles of a trim word: column groups of a rectangle
#define GSR_TRIM_MAX_UNITS 3     // row units it can take off either end of a column group
#define GSR_TRIM_K1 2.0f         // units of 2^-23 (ca cc + cb cb) by which the fp32 determinant may be off: gsr_rect_trim (1)
#define GSR_TRIM_K2 4.0f         // units of 2^-23 (ca X^2 + 2 |cb| X Y + cc Y^2) by which the fp32 `power` may be off, in q: gsr_rect_trim (2)

// log2 of the columns that share a nibble (w <= 8: 0) and of the rows per unit (h <= 16: 0): the smallest powers of two with
// at most 8 groups / at most 16 units
// (w <= 8 * 2^s  <=>  s >= log2(w) - 3: no loop -- pass 1's scatter decodes a word per Gaussian, and a data-dependent loop there cost it 10 us)
__host__ __device__ __forceinline__ uint32_t gsr_trim_col_shift(uint32_t w) { return w <= 8u ? 0u : 29u - (uint32_t)__builtin_clz(w - 1u); }
__host__ __device__ __forceinline__ uint32_t gsr_trim_row_shift(uint32_t h) { return h <= 16u ? 0u : 28u - (uint32_t)__builtin_clz(h - 1u); }

// rows taken off column c (< w) of a w x h rectangle: top (small y), bottom.  col_shift / row_shift: gsr_trim_col_shift(w), gsr_trim_row_shift(h)
__host__ __device__ __forceinline__ void gsr_trim_of(uint32_t trim, uint32_t c, uint32_t col_shift, uint32_t row_shift, uint32_t& top, uint32_t& bottom)
{
	const uint32_t nib = (trim >> (4u * ((c >> col_shift) & 7u))) & 15u;
	top = (nib & 3u) << row_shift;
	bottom = (nib >> 2) << row_shift;
}

// the columns of a w x h rectangle that keep at least one row: [lead, lead + wt).  (The producer leaves no empty column group between
// two kept ones -- gsr_rect_trim -- so that the kept columns are one run: the binning's histograms are difference arrays.)
__host__ __device__ __forceinline__ void gsr_trim_columns(uint32_t trim, uint32_t w, uint32_t h, uint32_t& lead, uint32_t& wt)
{
	lead = 0u; wt = w;
	if (trim == 0u || w == 0u) return;
	const uint32_t cs = gsr_trim_col_shift(w), rs = gsr_trim_row_shift(h);
	const uint32_t groups = (w + (1u << cs) - 1u) >> cs;
	uint32_t first = groups, last = 0u;
#pragma unroll
	for (uint32_t g = 0; g < (uint32_t)GSR_TRIM_GROUPS; g++) {
		uint32_t t, b;
		gsr_trim_of(trim, g << cs, cs, rs, t, b);
		if (g < groups && t + b < h) { first = first < g ? first : g; last = g + 1u; }
	}
	if (first >= last) { lead = 0u; wt = 0u; return; }
	lead = first << cs;
	wt = ((last << cs) < w ? (last << cs) : w) - lead;
}

#ifdef __HIPCC__
// The trim word of one Gaussian: centre (px, py) in pixel coordinates, conic (ca, cb, cc) and opacity as the blend kernels will read
// them from its record, rectangle [x0, x0 + w) x [y0, y0 + h) in tiles.  0 = nothing is taken off.
__device__ __forceinline__ uint32_t gsr_rect_trim(float px, float py, float ca, float cb, float cc, float opacity, int x0, int y0, int w, int h)
{
	if (w <= 0 || h <= 0) return 0u;
	const uint32_t cs = gsr_trim_col_shift((uint32_t)w), rs = gsr_trim_row_shift((uint32_t)h);
	const int groups = (int)(((uint32_t)w + (1u << cs) - 1u) >> cs);
	// (v_sqrt_f32 / v_rcp_f32 / v_log_f32 as they are, 1 ulp: the relative margins below are a thousand times that; the IEEE expansions of
	// sqrtf and of the division cost the geometry kernel, which the whole binning chain waits for, 7 us at 1 M Gaussians)
	// (1) The determinant.  T = ca cc and B = cb cb cancel: for a needle 1000 : 1 at 45 degrees to a few digits.  With u = 2^-24,
	// det0 = fl(fl(T) - fl(B)) = (fl(T) - fl(B)) (1 + d), |d| <= u, and |fl(T) - T| <= u T, |fl(B) - B| <= u B, so the exact
	// determinant of the three floats lies within u det0 + u (T + B) <= u T (1 + u) + u (T + B) of det0; forming the bound itself
	// (the sum, the product, the subtraction: 3 roundings, each <= u T (1 + 3 u)) adds less than another u (T + B):
	// |det - det0| < 3 u (T + B) = 1.5 * 2^-23 (T + B).  GSR_TRIM_K1 = 2 is the next whole number; what it leaves over
	// (2^-24 (T + B)) pays for the rounding of the fp32 sum T + B.  Every length below grows as det shrinks, so the LOWER end is used.
	const float det0 = ca * cc - cb * cb;
	const float dspan = (GSR_TRIM_K1 * 0x1p-23f) * (ca * cc + cb * cb);
	const float det = det0 - dspan;
	// (2) The threshold.  q = ca dx^2 + 2 cb dx dy + cc dy^2 <= 2 ln(255 opacity) is necessary for alpha >= 1 / 255 in exact
	// arithmetic.  The blend kernels decide with `power` = fl(fl(-0.5 fl(fl(fl(ca dx) dx) + fl(fl(cc dy) dy))) - fl(fl(cb dx) dy))
	// (gsr_pair_power, render_common.h; dx, dy the kernels' own rounded mean - pixel): four roundings on the way of the squares,
	// three on the way of the mixed term, so |-2 power - q| <= ((1 + u)^4 - 1) M = 2 * 2^-23 M (1 + 2 u) with
	// M = ca dx^2 + 2 |cb dx dy| + cc dy^2, the magnitude of what cancels.  M grows with |dx| and |dy|; it is taken at X, Y, the
	// largest |dx| and |dy| of the rectangle's pixel columns and rows (the same subtractions the kernels round).  GSR_TRIM_K2 = 4,
	// twice the bound: the other half pays for the seven roundings of M's own evaluation here and keeps the second-order terms out of the
	// argument.  For a splat of a few pixels this adds 1e-5 to tau; for a needle whose centre lies thousands of pixels off, M reaches
	// 1e6 and the term 0.5.  The constant part (0.1 % + 0.01 in q, 0.005 in `power`) remains for what has an absolute or a relative
	// error of a few u: v_log here, the kernels' exp and product (1e-6 of alpha), and the roundings of the lengths below -- of
	// tau cc - det lo^2 above all, whose error 6 u tau cc is 3e-4 of the 0.001 tau cc the margin adds to it.
	const float X = fmaxf(fabsf((float)(x0 * GSR_TILE_X) - px), fabsf((float)((x0 + w) * GSR_TILE_X - 1) - px));
	const float Y = fmaxf(fabsf((float)(y0 * GSR_TILE_Y) - py), fabsf((float)((y0 + h) * GSR_TILE_Y - 1) - py));
	const float tau0 = 2.0f * __logf(255.0f * opacity) * 1.001f + 0.01f;
	const float tau = tau0 + (GSR_TRIM_K2 * 0x1p-23f) * (ca * X * X + 2.0f * fabsf(cb) * X * Y + cc * Y * Y);
	if (!(det > 0.0f) || !(ca > 0.0f) || !(cc > 0.0f) || !(tau == tau)) return 0u;   // not an ellipse this bound understands (or one whose determinant is all rounding): keep everything
	uint32_t trim = 0u;
	uint32_t first = (uint32_t)groups, last = 0u;
	if (tau0 > 0.0f) {
		const float inv_det = __builtin_amdgcn_rcpf(det);
		const float ex = __builtin_amdgcn_sqrtf(tau * cc * inv_det) * 1.0001f + 0.01f;      // half width of the ellipse
		const float eyy = __builtin_amdgcn_sqrtf(tau * ca * inv_det) * 1.0001f + 0.01f;     // half height
		// dx of the ellipse's bottom point (largest dy), -cb sqrt(tau / (det ca)); its top point: the negative.  Only known as well as
		// det: it lies in [bx0, bx1], from det's upper end (det0 + dspan; sqrt(r) >= r for r <= 1 saves the second square root) to its
		// lower one.  (With the lower end in place of det the boundary below peaks at -cb sqrt(tau cc / (det (det + cb^2))) instead:
		// farther out by less than 1 + 8 u (ca cc + cb^2) / (det + cb^2) <= 1 + 2e-6, inside the 1e-4.)
		const float xs = fabsf(cb) * __builtin_amdgcn_sqrtf(tau * inv_det * __builtin_amdgcn_rcpf(ca));
		const float xs1 = xs * 1.0001f + 0.01f, xs0 = xs * (det * __builtin_amdgcn_rcpf(det0 + dspan)) * 0.9999f - 0.01f;
		const float bx0 = cb <= 0.0f ? xs0 : -xs1, bx1 = cb <= 0.0f ? xs1 : -xs0;
		const float inv_cc = __builtin_amdgcn_rcpf(cc);
#pragma unroll
		for (int c = 0; c < GSR_TRIM_GROUPS; c++) {
			if (c >= groups) break;
			// the strip of pixel centres of the tile columns of group c, relative to the centre, widened by the margin
			const int c0 = x0 + (c << cs), c1 = min(x0 + w, x0 + ((c + 1) << cs));   // tile columns [c0, c1)
			float lo = (float)(c0 * GSR_TILE_X) - px - 0.01f, hi = (float)(c1 * GSR_TILE_X - 1) - px + 0.01f;
			uint32_t t = GSR_TRIM_MAX_UNITS, b = GSR_TRIM_MAX_UNITS;   // the ellipse misses the strip: as much off as the word can say
			if (!(lo > ex) && !(hi < -ex)) {   // (written so that a NaN anywhere keeps the column whole: every comparison below is false then)
				lo = fmaxf(lo, -ex); hi = fminf(hi, ex);
				// largest dy over the strip: the ellipse's bottom point if its dx can lie inside, else at the nearer end (the boundary is
				// concave, and so is the one drawn with det's lower end, which lies outside it everywhere)
				const float rlo = __builtin_amdgcn_sqrtf(fmaxf(0.0f, tau * cc - det * lo * lo)), rhi = __builtin_amdgcn_sqrtf(fmaxf(0.0f, tau * cc - det * hi * hi));
				float ymax = fmaxf((-cb * lo + rlo) * inv_cc, (-cb * hi + rhi) * inv_cc);
				float ymin = fminf((-cb * lo - rlo) * inv_cc, (-cb * hi - rhi) * inv_cc);
				if (lo <= bx1 && bx0 <= hi) ymax = eyy;
				if (lo <= -bx0 && -bx1 <= hi) ymin = -eyy;
				ymax = ymax * 1.0001f + 0.01f;
				ymin = ymin * 1.0001f - 0.01f;
				// tile rows that hold a pixel centre in [py + ymin, py + ymax] -- or fewer: rows of the bounds themselves
				const float r0 = floorf((py + ymin) * (1.0f / GSR_TILE_Y)), r1 = floorf((py + ymax) * (1.0f / GSR_TILE_Y));
				// (fmaxf / fminf return their other operand for a NaN: 0 rows then)
				const float unit = 1.0f / (float)(1u << rs);   // whole units only: rounded down
				const float tf = fminf(floorf(fmaxf(r0 - (float)y0, 0.0f) * unit), (float)GSR_TRIM_MAX_UNITS);
				const float bf = fminf(floorf(fmaxf((float)(y0 + h - 1) - r1, 0.0f) * unit), (float)GSR_TRIM_MAX_UNITS);
				t = (uint32_t)tf; b = (uint32_t)bf;
			}
			trim |= (t | (b << 2)) << (4 * c);
			if (((t + b) << rs) < (uint32_t)h) { first = first < (uint32_t)c ? first : (uint32_t)c; last = (uint32_t)c + 1u; }
		}
	} else {
		// opacity below 1 / 255 (with the margin): alpha >= 1 / 255 nowhere
#pragma unroll
		for (int c = 0; c < GSR_TRIM_GROUPS; c++)
			if (c < groups) trim |= 15u << (4 * c);
	}
	// no empty column group between two kept ones (cannot happen for a convex shape; the decoder relies on it): give such a group back whole
#pragma unroll
	for (int c = 0; c < GSR_TRIM_GROUPS; c++)
		if ((uint32_t)c > first && (uint32_t)c + 1u < last) {
			const uint32_t nib = (trim >> (4 * c)) & 15u;
			if ((((nib & 3u) + (nib >> 2)) << rs) >= (uint32_t)h) trim &= ~(15u << (4 * c));
		}
	return trim;
}
#endif
