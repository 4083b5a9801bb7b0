// distortion.hip -- the depth-distortion map of a depth-and-alpha forward and its gradient (include/gsr_distortion.h):
//   Dist(p) = sum_{j<i} w_i w_j (v_i - v_j)^2,   w_i = alpha_i T_i the colour pass's own weights, v_i the record's depth value
// (the pairwise squared form of Mip-NeRF 360's distortion loss, as 2DGS and gsplat's `distloss` use it).  Two kernels, no atomics,
// no workgroup barrier, bitwise reproducible.  None of the default kernels is touched: both passes read the state an aux-mode
// forward left, the way contrib.hip and features.hip do, and v from the last word of the splat record.
//
// Both passes are the replay walk of gsr_replay.h; the payload is the record's depth word.
//
// Forward: front to back.  Per pixel a weighted Welford recurrence in list order keeps the sum centred:
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
// back to front, accum_rec of g h with a zero background, the straight-through 0.99 clamp: dL/dalpha_i = T_i (g h_i - accum_rec).
// Per (Gaussian, tile) instance with at least one hit the wave reduces seven values (gsr_row_reduce) -- the raw moments of
// f = G dL/dG and sum G dL/dalpha (gsr_pair_moments), and dL/dv = sum 2 g w A (v - mu) -- and ADDS the first six into words 0..5 of
// the GsrGradSlot the aux colour blend wrote for the same instance, the seventh into word 9 (pad0, the blend's own dL/dv), in one
// read-modify-write by lanes 0..6 (gsr_slot_add_geometry<true>).  The hit set is the colour blend's, so exactly the slots it
// validated are updated and the unchanged per-Gaussian aux backward chains the totals, word 9 along the view z axis.
// Seven values are 28 of the 64 reader lanes, so one instance is finished per round trip; the four-instance flush of
// render_backward.hip is laid out for 8 + 8 lanes per instance and nine values and would need a second layout for
// seven, for a pass that is bound by the per-pixel arithmetic.
//
// Registers (hipcc 7.x, gfx950, -O3 -ffp-contract=off; `make audit`, .audit/distortion.s): see DESIGN.md 6j.
#include "gsr_replay.h"

#define GSR_DIST_NV 7
#define GSR_DIST_ROWS 8     // rows of the reduction area: lane 4 v + q reads row v & 7

struct GsrDistForwardPass : GsrReplayPass {
	float A[GSR_PIX_PER_LANE], m[GSR_PIX_PER_LANE], S[GSR_PIX_PER_LANE];   // sum w, the weighted mean of v minus v0, sum w (v - mu)^2
	float v0[GSR_PIX_PER_LANE];                                            // v of the pixel's first hit
	__device__ __forceinline__ float load(uint32_t, const float4* p) const { return p[2].w; }   // the depth value v (aux-mode records)
	__device__ __forceinline__ float put(int, float v) const { return v; }                      // rides in rec[1].w
	__device__ __forceinline__ void pixel(const GsrTileWalk&, const GsrInstance& in, int k, float, const GsrPairFwd& p, None&)
	{
		// the Welford step; a pixel without a hit runs it with w = 0 and r = 0: the identity on (A, m, S), bit for bit
		const float v = in.B.w;
		v0[k] = (p.hit && A[k] == 0.f) ? v : v0[k];   // first hit: x = 0, d = 0, so m and S stay 0 exactly
		const float An = A[k] + p.w;
		const float r = p.hit ? p.w * __builtin_amdgcn_rcpf(An) : 0.0f;
		const float x = v - v0[k];
		const float d = x - m[k];
		m[k] = __builtin_fmaf(r, d, m[k]);
		S[k] = __builtin_fmaf(p.w * d, x - m[k], S[k]);
		A[k] = An;
	}
};

// declared for five waves per SIMD: at the six the allocator would take (80 VGPRs) the kernel measured 2 % slower
__global__ void __launch_bounds__(64 * GSR_WAVES_PER_WG) __attribute__((amdgpu_waves_per_eu(5, 5))) gsr_distortion_forward_kernel(
	int W, int H, int gx, int ntiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
	const GsrSplat* __restrict__ splat, const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max_contrib,
	float* __restrict__ out, float* __restrict__ state, int cull)
{
	__shared__ GsrBatchLds s_batch[GSR_WAVES_PER_WG];
	GsrTileWalk w;
	gsr_walk_tile(w, gx);
	if (w.tile >= ntiles) return;
	gsr_walk_list(w, ranges, point_list, tile_max_contrib);   // n = 0: the tile's pixels get zeros
	GsrDistForwardPass pass;
	gsr_walk_pixels<uint32_t>(w, W, H, n_contrib, nullptr, [&](int k, bool, uint32_t) {
		pass.A[k] = 0.f; pass.m[k] = 0.f; pass.S[k] = 0.f; pass.v0[k] = 0.f;
	});
	GSR_REPLAY(false, false, w, s_batch[w.wave], splat, (const uint32_t*)nullptr, cull, pass);

	const size_t plane = (size_t)H * W;
#pragma unroll
	for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
		if (w.px < W && w.py(k) < H) {
			const size_t pix_id = (size_t)W * w.py(k) + w.px;
			out[pix_id] = pass.A[k] * pass.S[k];
			state[pix_id] = pass.A[k];
			state[plane + pix_id] = pass.v0[k] + pass.m[k];
			state[2 * plane + pix_id] = pass.S[k];
		}
	}
}

struct GsrDistBackwardPass : GsrReplayPass {
	struct Acc {
		float v;                  // the instance's depth value
		// per-lane partial sums over its four pixels: [0..4] the raw moments of f = G dL/dG, [5] G dL/dalpha, [6] 2 g w A (v - mu)
		float s[GSR_DIST_NV];
		unsigned long long any;   // lanes with a hit
	};
	float ar[GSR_PIX_PER_LANE];    // accum_rec of g h as the NEXT hit will see it
	float g[GSR_PIX_PER_LANE];     // dL/dDist of the pixel
	float gA2[GSR_PIX_PER_LANE];   // 2 g A
	float A[GSR_PIX_PER_LANE], mu[GSR_PIX_PER_LANE], S[GSR_PIX_PER_LANE];   // the pixel's final state
	float* recv;                   // the wave's 64 staged depth values
	float* red;                    // the wave's reduction area
	GsrGradSlot* slots;
	float half_w, half_h;

	__device__ __forceinline__ float load(uint32_t, const float4* p) const { return p[2].w; }   // the depth value v (aux-mode records)
	__device__ __forceinline__ float put(int pos, float v) const { recv[pos] = v; return 0.f; }
	__device__ __forceinline__ Acc begin(const GsrInstance& in) const
	{
		Acc a = {recv[in.j], {}, 0ull};
		return a;
	}
	__device__ __forceinline__ void pixel(const GsrTileWalk&, const GsrInstance& in, int k, float dy, const GsrPairBwd& p, Acc& a)
	{
		a.any |= p.hitm;
		// the pixel's "feature": g h = g (A (v - mu)^2 + S); dL/dalpha = (g h - accum_rec) T
		const float dv = a.v - mu[k];
		const float h = __builtin_fmaf(A[k] * dv, dv, S[k]);
		const float d = g[k] * h - ar[k];
		// accum_rec' = alpha g h + (1 - alpha) accum_rec, on the difference above (render_backward.hip)
		ar[k] = __builtin_fmaf(p.alpha, d, ar[k]);
		const float dla = p.hit ? d * p.Tn : 0.f;   // (zero background: no T_final term)
		const float wgt = p.alpha * p.Tn;           // w; 0 without a hit
		a.s[6] = __builtin_fmaf(wgt * gA2[k], dv, a.s[6]);   // dL/dv
		gsr_pair_moments(a.s, a.s[5], in.B.y, p.G, dla, in.dx, dy);
	}
	__device__ __forceinline__ void finish(const GsrTileWalk& w, const GsrInstance& in, Acc& a) const
	{
		if (a.any == 0ull) return;   // wave-uniform: nothing is added for an instance without a hit
		float R[GSR_DIST_NV];   // wave-uniform
		gsr_row_reduce<GSR_DIST_NV, GSR_DIST_ROWS>(red, w.lane, a.s, R);
		gsr_slot_add_geometry<true>(slots, in.slot(), w.lane, in, half_w, half_h, R, R[5], R[6]);   // words 0..5, and pad0
	}
};

__global__ void __launch_bounds__(64 * GSR_WAVES_PER_WG) gsr_distortion_backward_kernel(
	int W, int H, int gx, int ntiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
	const GsrSplat* __restrict__ splat, const uint32_t* __restrict__ slot_base, const float* __restrict__ final_Ts,
	const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max_contrib, const float* __restrict__ state,
	const float* __restrict__ dL_ddist, GsrGradSlot* slots, int cull)
{
	__shared__ GsrBatchLds s_batch[GSR_WAVES_PER_WG];
	__shared__ float s_v[GSR_WAVES_PER_WG][64];
	__shared__ __attribute__((aligned(16))) float s_red[GSR_WAVES_PER_WG][GSR_DIST_ROWS * GSR_REPLAY_ROW];
	GsrTileWalk w;
	gsr_walk_tile(w, gx);
	if (w.tile >= ntiles) return;
	gsr_walk_list(w, ranges, point_list, tile_max_contrib);
	if (w.n <= 0) return;

	GsrDistBackwardPass pass;
	pass.recv = s_v[w.wave];
	pass.red = s_red[w.wave];
	pass.slots = slots;
	pass.half_w = 0.5f * W;
	pass.half_h = 0.5f * H;
	const size_t plane = (size_t)H * W;
	gsr_walk_pixels<size_t>(w, W, H, n_contrib, final_Ts, [&](int k, bool inside, size_t pix_id) {
		pass.ar[k] = 0.f;
		pass.g[k] = inside ? dL_ddist[pix_id] : 0.f;
		pass.A[k] = inside ? state[pix_id] : 0.f;
		pass.mu[k] = inside ? state[plane + pix_id] : 0.f;
		pass.S[k] = inside ? state[2 * plane + pix_id] : 0.f;
		pass.gA2[k] = 2.0f * pass.g[k] * pass.A[k];
	});
	GSR_REPLAY(true, true, w, s_batch[w.wave], splat, slot_base, cull, pass);
}

void gsr_launch_distortion_forward(const GsrFrame& f, float* out, float* state)
{
	const GsrTileGrid t = gsr_tile_grid(f.W, f.H);
	gsr_launch(gsr_distortion_forward_kernel, t.grid, t.block, 0, f.s, nullptr, nullptr, f.W, f.H, t.gx, t.ntiles, f.img.ranges, f.bin.point_list,
	           f.g.splat, f.img.n_contrib, f.img.tile_max_contrib, out, state, f.cull ? 1 : 0);
}

void gsr_launch_distortion_backward(const GsrFrame& f, const float* state, const float* dL_ddist)
{
	const GsrTileGrid t = gsr_tile_grid(f.W, f.H);
	gsr_launch(gsr_distortion_backward_kernel, t.grid, t.block, 0, f.s, nullptr, nullptr, f.W, f.H, t.gx, t.ntiles, f.img.ranges, f.bin.point_list,
	           f.g.splat, f.g.slot_base, f.img.final_T, f.img.n_contrib, f.img.tile_max_contrib, state, dL_ddist, f.slots, f.cull ? 1 : 0);
}
