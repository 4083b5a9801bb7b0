// distortion.hip -- the depth-distortion map of a depth-and-alpha forward and its gradient (include/gsr_distortion.h):
//   Dist(p) = sum_{j<i} w_i w_j (v_i - v_j)^2,   w_i = alpha_i T_i the colour pass's own weights, v_i the record's depth value
// (the pairwise squared form of Mip-NeRF 360's distortion loss, as 2DGS and gsplat's `distloss` use it).  Two kernels, no atomics,
// no workgroup barrier, bitwise reproducible.  None of the default kernels is touched: both passes read the state an aux-mode
// forward left, the way contrib.hip and features.hip do, and v from the last word of the splat record.
//
// Decomposition (render_common.h): one wave64 per 16x16 tile, four pixels per lane, 64 instances staged per batch into the wave's LDS
// slice behind gsr_tile_band_mask (`cull`).
//
// Forward: the forward's walk over again, exactly as gsr_features_forward_kernel walks it (list positions
// [0, min(range length, tile_max_contrib)), per pixel only those in front of its n_contrib; `power`, alpha, the two thresholds and
// T's update are render_forward.hip's instruction sequence on the same records), so w has the colour pass's bits.  Per pixel a
// weighted Welford recurrence in list order keeps the sum centred:
//   A' = A + w,  d = v - mu,  mu' = mu + (w / A') d,  S' = S + w d (v - mu'),  Dist = A S
// (S = sum w (v - mu)^2 and sum_{j<i} w_i w_j (v_i - v_j)^2 = A S).  The mean is carried relative to the pixel's first blended depth
// v0, m = mu - v0: v - v0 is exact in fp32 for depths of one ray, so the recurrence rounds at the size of the ray's spread, not of
// the depths (carried as mu itself every step rounds at ulp(v): measured 1.3e-5 against 3.3e-7 on a map of size 1 at depths of 50), and mu = v0 + m is
// formed once, for the state.  A pixel with one Gaussian has m = 0, S = 0 and Dist = 0 exactly.  w / A' is w * v_rcp_f32(A'): its
// one ulp moves mu' by an ulp of the step, never the centring.  The raw moments sum w v, sum w v^2 are not formed anywhere.
// Written in full: Dist [H][W] and the state planes A, mu, S ([3][H][W]), zeros where nothing blends.
//
// Backward: features.hip's backward tile pass with ONE channel whose "feature" is computed per pixel, g h_i with
//   h_i = dDist/dw_i = A (v_i - mu)^2 + S          (the pixel's final A, mu, S)
// back to front from final_T and n_contrib, T_i = T_{i+1} / (1 - alpha_i) (v_rcp_f32), accum_rec of g h with a zero background, the
// straight-through 0.99 clamp: dL/dalpha_i = T_i (g h_i - accum_rec).  Per (Gaussian, tile) instance with at least one hit the wave
// reduces seven values -- the raw moments sum f dx, f dy, f dx^2, f dx dy, f dy^2 of f = G dL/dG, sum G dL/dalpha, and
// dL/dv = sum 2 g w A (v - mu) -- finishes the first six with render_backward.hip's epilogue algebra and ADDS them into words 0..5
// of the GsrGradSlot the aux colour blend wrote for the same instance, the seventh into word 9 (pad0, the blend's own dL/dv): a
// plain read-modify-write by lanes 0..6 of the one wave that owns the tile.  The hit set is the colour blend's (same records, same
// n_contrib, same thresholds), so exactly the slots it validated are updated and the unchanged per-Gaussian aux backward chains
// the totals, word 9 along the view z axis.
// Reduction: the per-instance LDS rows of features.hip -- each lane stores its 7 partials into 7 rows of 64 words
// (row stride 80), lane 4 v + q folds quarter q of row v & 7 with four ds_read_b128, two lane exchanges join the quarters, the totals
// are broadcast as scalars for the epilogue.  Seven values are 28 of the 64 reader lanes, so one instance is finished per round trip
// as there; the four-instance flush of render_backward.hip is laid out for 8 + 8 lanes per instance and nine values
// and would need a second layout for seven, for a pass that is bound by the per-pixel arithmetic.
// Heavy tiles are walked whole by one wave (no depth segments), as the feature pass walks them.
//
// Registers (hipcc 7.x, gfx950, -O3 -ffp-contract=off; `make audit`, .audit/distortion.s): see DESIGN.md 6j.
#include "render_common.h"

#define GSR_DIST_NV 7
#define GSR_DIST_ROW 80     // words between two rows of the reduction area (features.hip GSR_FEAT_ROW)
#define GSR_DIST_ROWS 8     // rows allocated: lane 4 v + q reads row v & 7

__global__ void __launch_bounds__(64 * GSR_WAVES_PER_WG) gsr_distortion_forward_kernel(
	int W, int H, int gx, int ntiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
	const GsrSplat* __restrict__ splat, const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max_contrib,
	float* __restrict__ out, float* __restrict__ state, int cull)
{
	// the surviving instances of a batch: (x, y, -0.5 conic a, conic b), (-0.5 conic c, opacity, list position, v)
	__shared__ float4 s_rec[GSR_WAVES_PER_WG][2][64];
	__shared__ uint32_t s_bands[GSR_WAVES_PER_WG][64];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int tile = blockIdx.x * GSR_WAVES_PER_WG + wave;
	if (tile >= ntiles) return;  // wave-uniform; no barriers below
	float4(*rec)[64] = s_rec[wave];
	uint32_t* recb = s_bands[wave];

	const int tx = tile % gx, ty = tile / gx;
	const int px = tx * GSR_TILE_X + (lane & 15);
	const int py0 = ty * GSR_TILE_Y + (lane >> 4);
	const float pfx = (float)px;
	const float x0f = (float)(tx * GSR_TILE_X), y0f = (float)(ty * GSR_TILE_Y);

	const uint2 range = ranges[tile];
	const int n = (int)min(range.y - range.x, tile_max_contrib[tile]);  // the tail was never blended; 0: the tile's pixels get zeros
	const uint32_t* plist = point_list + range.x;

	float T[GSR_PIX_PER_LANE], pfy[GSR_PIX_PER_LANE];
	float A[GSR_PIX_PER_LANE], m[GSR_PIX_PER_LANE], S[GSR_PIX_PER_LANE];   // sum w, the weighted mean of v minus v0, sum w (v - mu)^2
	float v0[GSR_PIX_PER_LANE];             // v of the pixel's first hit
	uint32_t last[GSR_PIX_PER_LANE];        // the pixel's n_contrib: it blended positions in front of this one only (0 outside the image)
	uint32_t band_last[GSR_PIX_PER_LANE];   // wave-uniform: the largest of them in band k
#pragma unroll
	for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
		const int py = py0 + 4 * k;
		const bool inside = px < W && py < H;
		const uint32_t pix_id = inside ? (uint32_t)(W * py + px) : 0u;
		pfy[k] = (float)py;
		T[k] = 1.0f;
		A[k] = 0.f; m[k] = 0.f; S[k] = 0.f; v0[k] = 0.f;
		last[k] = inside ? n_contrib[pix_id] : 0u;
		uint32_t lm = last[k];
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) lm = max(lm, (uint32_t)__shfl_xor((int)lm, off, 64));
		band_last[k] = __builtin_amdgcn_readfirstlane(lm);
	}

	// software pipeline: records one batch ahead, ids two batches ahead
	float4 ra = make_float4(0, 0, 0, 0), rb = ra;
	float rv = 0.f;
	if (lane < n) {
		const uint32_t id = plist[lane];
		const float4* p = reinterpret_cast<const float4*>(splat + id);
		ra = p[0]; rb = p[1];
		rv = p[2].w;   // the depth value v (aux-mode records)
	}
	uint32_t id_next = (64 + lane < n) ? plist[64 + lane] : 0u;

	for (int base = 0; base < n; base += 64) {
		const uint32_t bands = (base + lane < n) ? (cull ? gsr_tile_band_mask(ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, x0f, y0f) : 0xFu) : 0u;
		const bool keep = bands != 0u;
		const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
		const int cnt = __popcll(mask);
		if (keep) {
			const int pos = gsr_mbcnt(mask);
			rec[0][pos] = make_float4(ra.x, ra.y, -0.5f * ra.z, ra.w);  // conic a, c pre-multiplied by -0.5 (exact)
			rec[1][pos] = make_float4(-0.5f * rb.x, rb.y, __uint_as_float((uint32_t)(base + lane)), rv);
			recb[pos] = bands;
		}
		if (base + 64 + lane < n) {
			const float4* p = reinterpret_cast<const float4*>(splat + id_next);
			ra = p[0]; rb = p[1];
			rv = p[2].w;
		}
		id_next = (base + 128 + lane < n) ? plist[base + 128 + lane] : 0u;
		__builtin_amdgcn_wave_barrier();

		for (int j = 0; j < cnt; j++) {
			const float4 RA = rec[0][j];   // x, y, -0.5 conic a, conic b
			const float4 RB = rec[1][j];   // -0.5 conic c, opacity, list position, v
			const uint32_t position = __builtin_amdgcn_readfirstlane(__float_as_uint(RB.z));   // wave-uniform
			const uint32_t jbands = __builtin_amdgcn_readfirstlane(recb[j]);                  // wave-uniform
			const float v = RB.w;
			const float dx = RA.x - pfx;
			const float ax2 = __fmul_rn(__fmul_rn(RA.z, dx), dx), bdx = __fmul_rn(RA.w, dx);
#pragma unroll
			for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
				if (!(jbands & (1u << k)) || position >= band_last[k]) continue;  // scalar branch: the band cannot be reached, or it had finished
				const float dy = RA.y - pfy[k];
				const float power = gsr_pair_power_halved(ax2, bdx, RB.x, dy);
				const float alpha = fminf(0.99f, RB.y * __expf(power));
				const unsigned long long hitm = __builtin_amdgcn_ballot_w64(position < last[k]) & __builtin_amdgcn_ballot_w64(!(power > 0.0f)) &
				                                __builtin_amdgcn_ballot_w64(!(alpha < 1.0f / 255.0f));
				if (hitm == 0ull) continue;  // wave-uniform
				const bool hit = __builtin_amdgcn_inverse_ballot_w64(hitm);
				const float w = hit ? __fmul_rn(alpha, T[k]) : 0.0f;                  // the forward's alpha * T
				T[k] = hit ? __fmul_rn(T[k], __fsub_rn(1.0f, alpha)) : T[k];          // ... and its T (1 - alpha), rounded as there
				// the Welford step; a pixel without a hit runs it with w = 0 and r = 0: the identity on (A, m, S), bit for bit
				v0[k] = (hit && A[k] == 0.f) ? v : v0[k];   // first hit: x = 0, d = 0, so m and S stay 0 exactly
				const float An = A[k] + w;
				const float r = hit ? w * __builtin_amdgcn_rcpf(An) : 0.0f;
				const float x = v - v0[k];
				const float d = x - m[k];
				m[k] = __builtin_fmaf(r, d, m[k]);
				S[k] = __builtin_fmaf(w * d, x - m[k], S[k]);
				A[k] = An;
			}
		}
		__builtin_amdgcn_wave_barrier();
	}

	const size_t plane = (size_t)H * W;
#pragma unroll
	for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
		const int py = py0 + 4 * k;
		if (px < W && py < H) {
			const size_t pix_id = (size_t)W * py + px;
			out[pix_id] = A[k] * S[k];
			state[pix_id] = A[k];
			state[plane + pix_id] = v0[k] + m[k];
			state[2 * plane + pix_id] = S[k];
		}
	}
}

__global__ void __launch_bounds__(64 * GSR_WAVES_PER_WG) gsr_distortion_backward_kernel(
	int W, int H, int gx, int ntiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
	const GsrSplat* __restrict__ splat, const uint32_t* __restrict__ slot_base, const float* __restrict__ final_Ts,
	const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max_contrib, const float* __restrict__ state,
	const float* __restrict__ dL_ddist, GsrGradSlot* slots, int cull)
{
	// the surviving instances of a batch: (x, y, -0.5 conic a, conic b), (-0.5 conic c, opacity, list position, slot), v
	__shared__ float4 s_rec[GSR_WAVES_PER_WG][2][64];
	__shared__ float s_v[GSR_WAVES_PER_WG][64];
	__shared__ uint32_t s_bands[GSR_WAVES_PER_WG][64];
	// reduction area: row i holds the 64 lanes' partial i of the instance being reduced
	__shared__ __attribute__((aligned(16))) float s_red[GSR_WAVES_PER_WG][GSR_DIST_ROWS * GSR_DIST_ROW];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int tile = blockIdx.x * GSR_WAVES_PER_WG + wave;
	if (tile >= ntiles) return;  // wave-uniform; no barriers below
	float4(*rec)[64] = s_rec[wave];
	float* recv = s_v[wave];
	uint32_t* recb = s_bands[wave];
	float* red = s_red[wave];

	const int tx = tile % gx, ty = tile / gx;
	const int px = tx * GSR_TILE_X + (lane & 15);
	const int py0 = ty * GSR_TILE_Y + (lane >> 4);
	const float pfx = (float)px;
	const float x0f = (float)(tx * GSR_TILE_X), y0f = (float)(ty * GSR_TILE_Y);

	const uint2 range = ranges[tile];
	const int n = (int)min(range.y - range.x, tile_max_contrib[tile]);  // the tail was never blended
	if (n <= 0) return;
	const uint32_t* plist = point_list + range.x;
	const size_t plane = (size_t)H * W;
	const float ddelx_dx = 0.5f * W, ddely_dy = 0.5f * H;

	float T[GSR_PIX_PER_LANE], pfy[GSR_PIX_PER_LANE];
	float ar[GSR_PIX_PER_LANE];    // accum_rec of g h as the NEXT hit will see it
	float g[GSR_PIX_PER_LANE];     // dL/dDist of the pixel
	float gA2[GSR_PIX_PER_LANE];   // 2 g A
	float A[GSR_PIX_PER_LANE], mu[GSR_PIX_PER_LANE], S[GSR_PIX_PER_LANE];   // the pixel's final state
	uint32_t last[GSR_PIX_PER_LANE], band_last[GSR_PIX_PER_LANE];
#pragma unroll
	for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
		const int py = py0 + 4 * k;
		const bool inside = px < W && py < H;
		const size_t pix_id = inside ? (size_t)W * py + px : 0;
		pfy[k] = (float)py;
		T[k] = inside ? final_Ts[pix_id] : 0.f;
		last[k] = inside ? n_contrib[pix_id] : 0u;
		ar[k] = 0.f;
		g[k] = inside ? dL_ddist[pix_id] : 0.f;
		A[k] = inside ? state[pix_id] : 0.f;
		mu[k] = inside ? state[plane + pix_id] : 0.f;
		S[k] = inside ? state[2 * plane + pix_id] : 0.f;
		gA2[k] = 2.0f * g[k] * A[k];
		uint32_t m = last[k];
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
		band_last[k] = __builtin_amdgcn_readfirstlane(m);
	}

	// back to front: batch position q = base + lane maps to list position n - 1 - q
	float4 ra = make_float4(0, 0, 0, 0), rb = ra;
	float rv = 0.f;
	uint32_t sbase = 0u;
	if (lane < n) {
		const uint32_t id = plist[n - 1 - lane];
		const float4* p = reinterpret_cast<const float4*>(splat + id);
		ra = p[0]; rb = p[1];
		rv = p[2].w;   // the depth value v (aux-mode records)
		sbase = slot_base[id];
	}
	uint32_t id_next = (64 + lane < n) ? plist[n - 1 - (64 + lane)] : 0u;
	// the reduction's reader: lane 4 v + q folds the words 16 q .. 16 q + 15 of row v & 7
	const float* const red_r = red + ((lane >> 2) & 7) * GSR_DIST_ROW + 16 * (lane & 3);

	for (int base = 0; base < n; base += 64) {
		const uint32_t bands = (base + lane < n) ? (cull ? gsr_tile_band_mask(ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, x0f, y0f) : 0xFu) : 0u;
		const bool keep = bands != 0u;
		const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
		const int cnt = __popcll(mask);
		if (keep) {
			const int pos = gsr_mbcnt(mask);
			const uint32_t rmin = __float_as_uint(rb.z), rwh = __float_as_uint(rb.w);
			const uint32_t slot = sbase + ((uint32_t)ty - (rmin >> 16)) * (rwh & 0xffffu) + ((uint32_t)tx - (rmin & 0xffffu));
			rec[0][pos] = make_float4(ra.x, ra.y, -0.5f * ra.z, ra.w);  // conic a, c pre-multiplied by -0.5 (exact)
			rec[1][pos] = make_float4(-0.5f * rb.x, rb.y, __uint_as_float((uint32_t)(n - 1 - (base + lane))), __uint_as_float(slot));
			recv[pos] = rv;
			recb[pos] = bands;
		}
		if (base + 64 + lane < n) {
			const float4* p = reinterpret_cast<const float4*>(splat + id_next);
			ra = p[0]; rb = p[1];
			rv = p[2].w;
			sbase = slot_base[id_next];
		}
		id_next = (base + 128 + lane < n) ? plist[n - 1 - (base + 128 + lane)] : 0u;
		__builtin_amdgcn_wave_barrier();

		for (int j = 0; j < cnt; j++) {
			const float4 RA = rec[0][j];   // x, y, -0.5 conic a, conic b
			const float4 RB = rec[1][j];   // -0.5 conic c, opacity, list position, slot
			const float v = recv[j];
			const uint32_t position = __builtin_amdgcn_readfirstlane(__float_as_uint(RB.z));   // backward.cu:511-515; wave-uniform
			const uint32_t jbands = __builtin_amdgcn_readfirstlane(recb[j]);                  // wave-uniform
			const float dx = RA.x - pfx;
			const float ax2 = __fmul_rn(__fmul_rn(RA.z, dx), dx), bdx = __fmul_rn(RA.w, dx);
			// per-lane partial sums over its four pixels: [0..4] the raw moments of f = G dL/dG (f dx, f dy, f dx^2, f dx dy, f dy^2),
			// [5] G dL/dalpha, [6] 2 g w A (v - mu)
			float acc[GSR_DIST_NV];
#pragma unroll
			for (int i = 0; i < GSR_DIST_NV; i++) acc[i] = 0.f;
			unsigned long long any = 0ull;  // lanes with a hit
#pragma unroll
			for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
				if (!(jbands & (1u << k)) || position >= band_last[k]) continue;  // scalar branch: the band cannot be reached, or none of its pixels blended this far
				const float dy = RA.y - pfy[k];
				const float power = gsr_pair_power_halved(ax2, bdx, RB.x, dy);
				const float G = __expf(power);
				const float araw = fminf(0.99f, RB.y * G);
				const unsigned long long hitm = __builtin_amdgcn_ballot_w64(position < last[k]) & __builtin_amdgcn_ballot_w64(!(power > 0.0f)) &
				                                __builtin_amdgcn_ballot_w64(!(araw < 1.0f / 255.0f));
				if (hitm == 0ull) continue;  // wave-uniform
				any |= hitm;
				const bool hit = __builtin_amdgcn_inverse_ballot_w64(hitm);
				// a pixel that did not hit runs the same update with alpha = 0: the identity on its state, bit for bit
				const float alpha = hit ? araw : 0.f;
				const float inv1ma = __builtin_amdgcn_rcpf(1.f - alpha);
				const float Tn = T[k] * inv1ma;   // T in front of this instance
				// the pixel's "feature": g h = g (A (v - mu)^2 + S); dL/dalpha = (g h - accum_rec) T
				const float dv = v - mu[k];
				const float h = __builtin_fmaf(A[k] * dv, dv, S[k]);
				const float d = g[k] * h - ar[k];
				// accum_rec' = alpha g h + (1 - alpha) accum_rec, on the difference above (render_backward.hip)
				ar[k] = __builtin_fmaf(alpha, d, ar[k]);
				const float dla = hit ? d * Tn : 0.f;   // (zero background: no T_final term)
				const float wgt = alpha * Tn;           // w; 0 without a hit
				T[k] = Tn;
				acc[6] = __builtin_fmaf(wgt * gA2[k], dv, acc[6]);   // dL/dv
				acc[5] = __builtin_fmaf(G, dla, acc[5]);             // dL/dopacity
				const float f = (RB.y * dla) * G;                    // dL/dG * G (straight through the 0.99 clamp)
				const float fdx = f * dx, fdy = f * dy;
				acc[0] += fdx;
				acc[1] += fdy;
				acc[2] = __builtin_fmaf(fdx, dx, acc[2]);
				acc[3] = __builtin_fmaf(fdx, dy, acc[3]);
				acc[4] = __builtin_fmaf(fdy, dy, acc[4]);
			}
			if (any == 0ull) continue;   // wave-uniform: nothing is added for an instance without a hit
			// the wave reduction.  A wave's LDS operations execute in program order: the reads see all 64 lanes' stores, and the
			// next instance's stores come after them; the wave barriers keep the compiler from moving LDS accesses across.
#pragma unroll
			for (int i = 0; i < GSR_DIST_NV; i++) red[i * GSR_DIST_ROW + lane] = acc[i];
			__builtin_amdgcn_wave_barrier();
			const float4 q0 = *reinterpret_cast<const float4*>(red_r), q1 = *reinterpret_cast<const float4*>(red_r + 4);
			const float4 q2 = *reinterpret_cast<const float4*>(red_r + 8), q3 = *reinterpret_cast<const float4*>(red_r + 12);
			__builtin_amdgcn_wave_barrier();
			float t = (((q0.x + q0.y) + (q0.z + q0.w)) + ((q1.x + q1.y) + (q1.z + q1.w))) + (((q2.x + q2.y) + (q2.z + q2.w)) + ((q3.x + q3.y) + (q3.z + q3.w)));
			t += __shfl_xor(t, 1, 64);
			t += __shfl_xor(t, 2, 64);   // lanes 4 i .. 4 i + 3 hold the wave's total of value i (i = 7, and the lanes above 31: never used)
			float R[GSR_DIST_NV];   // wave-uniform
#pragma unroll
			for (int i = 0; i < GSR_DIST_NV; i++) R[i] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(t), 4 * i));
			const uint32_t slot = __builtin_amdgcn_readfirstlane(__float_as_uint(RB.w));
			// render_backward.hip's epilogue: dL/dmean2D = -0.5 W (a sx + b sy), -0.5 H (c sy + b sx), with a = -2 (-0.5 a)
			// inside the FMA; dL/dconic .x .y .w = -0.5 x the second moments; dL/dopacity and dL/dv as they are
			const float ca = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(RA.z)));
			const float cb = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(RA.w)));
			const float cc = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(RB.x)));
			const float r0 = -ddelx_dx * __builtin_fmaf(-2.0f, ca * R[0], cb * R[1]);
			const float r1 = -ddely_dy * __builtin_fmaf(-2.0f, cc * R[1], cb * R[0]);
			const float r = lane == 0 ? r0 : lane == 1 ? r1 : lane == 2 ? -0.5f * R[2] : lane == 3 ? -0.5f * R[3] : lane == 4 ? -0.5f * R[4] : lane == 5 ? R[5] : R[6];
			if (lane < GSR_DIST_NV) {
				float* w = reinterpret_cast<float*>(slots + slot) + (lane == 6 ? 9 : lane);   // words 0..5, and pad0
				*w = *w + r;
			}
		}
		__builtin_amdgcn_wave_barrier();
	}
}

void gsr_launch_distortion_forward(int W, int H, GsrImage img, const uint32_t* point_list, const GsrSplat* splat, float* out, float* state,
                                   bool cull, hipStream_t s)
{
	const int gx = gsr_grid_x(W), ntiles = gx * gsr_grid_y(H);
	gsr_launch(gsr_distortion_forward_kernel, dim3((ntiles + GSR_WAVES_PER_WG - 1) / GSR_WAVES_PER_WG), dim3(64 * GSR_WAVES_PER_WG), 0, s, nullptr,
	           nullptr, W, H, gx, ntiles, img.ranges, point_list, splat, img.n_contrib, img.tile_max_contrib, out, state, cull ? 1 : 0);
}

void gsr_launch_distortion_backward(int W, int H, GsrImage img, const uint32_t* point_list, const GsrSplat* splat, const uint32_t* slot_base,
                                    const float* state, const float* dL_ddist, GsrGradSlot* slots, bool cull, hipStream_t s)
{
	const int gx = gsr_grid_x(W), ntiles = gx * gsr_grid_y(H);
	gsr_launch(gsr_distortion_backward_kernel, dim3((ntiles + GSR_WAVES_PER_WG - 1) / GSR_WAVES_PER_WG), dim3(64 * GSR_WAVES_PER_WG), 0, s, nullptr,
	           nullptr, W, H, gx, ntiles, img.ranges, point_list, splat, slot_base, img.final_T, img.n_contrib, img.tile_max_contrib, state,
	           dL_ddist, slots, cull ? 1 : 0);
}
