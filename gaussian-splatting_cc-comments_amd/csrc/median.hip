// median.hip -- the median-depth map and the per-pixel Gaussian index maps of a forward, and the median depth's gradient
// (include/gsr_median.h).  For pixel p, over its blended Gaussians in list order, T_i the transmittance in front of Gaussian i and
// w_i = alpha_i T_i:
//   median(p)   = the LAST blended Gaussian with T_i > 0.5 (2DGS: `if (T > 0.5) median = this`, before T is updated)
//   dominant(p) = the FIRST blended Gaussian with the largest w_i (strict >)
// Two kernels, no atomics, no workgroup barrier, bitwise reproducible.  None of the default kernels is touched: both passes read the
// state a forward left, the way contrib.hip, features.hip and distortion.hip do.
//
// Forward: the replay walk of gsr_replay.h, front to back, no payload: every decision and every w has the colour pass's bits.  Per
// hit, with T the value in front of the hit:
//   if (T > 0.5) med = position;      w = alpha T;      if (w > best) { best = w; best_pos = position; }
// Only list positions are carried; the Gaussian ids (point_list[range.x + position]) and the median's depth value v (the last word of
// its splat record, the record's bits) are gathered once per pixel at the end -- two loads per pixel instead of a staged word and a
// select per hit.  Outputs that were not requested (NULL) cost no stores and no gathers.  The state plane [H][W] of uint32 holds the
// median's list position (0xFFFFFFFF: nothing blended) for the backward.
//
// Early exit (template argument EXIT; the twin without it is launched for GSR_DEBUG_MEDIAN_FULL_WALK).  After every batch a band whose
// every pixel is finished stops: a pixel is finished when it has no position left in front of its n_contrib, or when T <= 0.5 and
// T <= best.  Proof that the full walk changes nothing more for such a pixel.  Let T be its transmittance after the batch and T', alpha'
// those of any later hit.  (i) T' <= T: every update is T <- fmul_rn(T, fsub_rn(1, alpha)) with 0 < fsub_rn(1, alpha) < 1 (alpha in
// [1/255, 0.99]); the exact product is below T, T is representable, and rounding to nearest is monotone, so the rounded product is <= T.
// (ii) The median test of a later hit is T' > 0.5, false by T' <= T <= 0.5: med keeps its value.  (iii) Its weight is
// w' = fmul_rn(alpha', T') with alpha' <= 0.99 < 1: the exact product is below T', so w' <= T' <= T <= best, and the strict w' > best
// is false: best and best_pos keep their values.  T itself is not an output.  A band is skipped by setting its wave-uniform
// band_last to 0, the test the walk already makes per instance; the batch loop ends when no band is left.  Hence bit-identical outputs,
// and tests compare the two instantiations.
//
// Backward: dL/dv_i = sum_{p : median(p) = i} g(p), nothing through alpha or T (the choice of i is piecewise constant).  No alpha is
// recomputed and no list is walked: the wave reads its 256 state positions and g, and loops over the DISTINCT positions present (at
// most 256; 88 over the four tiles of the 32x32 test scene) instead of the tile's list (hundreds to thousands of instances, each with a
// staged record, a band test and the pair arithmetic on four pixels): per distinct position q one ballot, one readlane, four selects
// and a six-step xor butterfly of the lanes' partial sums -- a fixed order, every lane ends with the same bits.  The
// (q, total) pairs go to the wave's LDS; then lane l takes pairs l, l + 64, ...: id = point_list[range.x + q], the slot as
// distortion.hip forms it (slot_base[id] plus the rect offset from the record), and one read-modify-write of word 9 (pad0, the aux
// blend's own dL/dv).  Distinct positions of one tile are distinct Gaussians, so distinct slots: each (Gaussian, tile) slot receives
// at most one addition per launch and the order across instances is irrelevant.  The median blended, so its slot is one the colour
// blend validated; the unchanged aux per-Gaussian backward chains word 9 along the view z axis.  Heavy tiles are one wave like any other.
//
// Registers (hipcc 7.x, gfx950, -O3 -ffp-contract=off; `make audit`, .audit/median.s): see DESIGN.md 6k.
#include "gsr_replay.h"

#define GSR_MEDIAN_NONE 0xFFFFFFFFu

template <bool EXIT>
struct GsrMedianPass : GsrReplayPass {
	float best[GSR_PIX_PER_LANE];      // the largest w so far
	uint32_t med[GSR_PIX_PER_LANE];    // list position of the last hit with T > 0.5
	uint32_t bpos[GSR_PIX_PER_LANE];   // list position of the first hit with w = best
	__device__ __forceinline__ void pixel(const GsrTileWalk&, const GsrInstance& in, int k, float, const GsrPairFwd& p, None&)
	{
		med[k] = (p.hit && p.Tfront > 0.5f) ? in.position : med[k];
		const bool better = p.w > best[k];   // w = 0 without a hit never beats best >= 0
		best[k] = better ? p.w : best[k];
		bpos[k] = better ? in.position : bpos[k];
	}
	// EXIT: a band stops once each of its pixels has blended its last position or can change no more (the proof is in the header);
	// band_last = 0 is the test the walk already makes per instance
	__device__ __forceinline__ bool batch_done(GsrTileWalk& w, uint32_t next) const
	{
		if (!EXIT) return true;
		bool any = false;
#pragma unroll
		for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
			if (w.band_last[k] <= next) continue;   // finished, here or by its n_contrib
			const bool open = next < w.last[k] && (w.T[k] > 0.5f || w.T[k] > best[k]);
			if (__builtin_amdgcn_ballot_w64(open) == 0ull) w.band_last[k] = 0u;
			else any = true;
		}
		return any;   // wave-uniform
	}
};

// each twin is declared for its occupancy: left to itself the allocator takes 82 VGPRs for the full walk, a wave less
template <bool EXIT>
__global__ void __launch_bounds__(64 * GSR_WAVES_PER_WG) __attribute__((amdgpu_waves_per_eu(EXIT ? 5 : 6))) gsr_median_forward_kernel(
	int W, int H, int gx, int ntiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
	const GsrSplat* __restrict__ splat, const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max_contrib,
	float* __restrict__ out_depth, int32_t* __restrict__ out_median, int32_t* __restrict__ out_dominant, float* __restrict__ out_weight,
	uint32_t* __restrict__ state, int cull)
{
	__shared__ GsrBatchLds s_batch[GSR_WAVES_PER_WG];
	GsrTileWalk w;
	gsr_walk_tile(w, gx);
	if (w.tile >= ntiles) return;
	gsr_walk_list(w, ranges, point_list, tile_max_contrib);   // n = 0: the tile's pixels get "none"
	GsrMedianPass<EXIT> pass;
	gsr_walk_pixels<uint32_t>(w, W, H, n_contrib, nullptr, [&](int k, bool, uint32_t) {
		pass.best[k] = 0.f;
		pass.med[k] = GSR_MEDIAN_NONE; pass.bpos[k] = GSR_MEDIAN_NONE;
	});
	GSR_REPLAY(false, false, w, s_batch[w.wave], splat, (const uint32_t*)nullptr, cull, pass);

#pragma unroll
	for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
		if (w.px < W && w.py(k) < H) {
			const size_t pix_id = (size_t)W * w.py(k) + w.px;
			const bool some = pass.med[k] != GSR_MEDIAN_NONE;   // one hit sets both positions: the first hit has T = 1 and w > 0
			if (state) state[pix_id] = pass.med[k];
			if (out_depth || out_median) {
				const uint32_t id = some ? w.plist[pass.med[k]] : 0u;
				if (out_median) out_median[pix_id] = some ? (int32_t)id : -1;
				if (out_depth) out_depth[pix_id] = some ? reinterpret_cast<const float*>(splat + id)[11] : 0.f;   // the record's v
			}
			if (out_dominant) out_dominant[pix_id] = some ? (int32_t)w.plist[pass.bpos[k]] : -1;
			if (out_weight) out_weight[pix_id] = pass.best[k];
		}
	}
}

__global__ void __launch_bounds__(64 * GSR_WAVES_PER_WG) gsr_median_backward_kernel(
	int W, int H, int gx, int ntiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
	const GsrSplat* __restrict__ splat, const uint32_t* __restrict__ slot_base, const uint32_t* __restrict__ state,
	const float* __restrict__ dL_dmedian, GsrGradSlot* slots)
{
	// the distinct median positions of the tile and the sum of g over the pixels of each
	__shared__ uint32_t s_q[GSR_WAVES_PER_WG][256];
	__shared__ float s_t[GSR_WAVES_PER_WG][256];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int tile = blockIdx.x * GSR_WAVES_PER_WG + wave;
	if (tile >= ntiles) return;  // wave-uniform; no barriers below
	uint32_t* sq = s_q[wave];
	float* stot = s_t[wave];

	const int tx = tile % gx, ty = tile / gx;
	const int px = tx * GSR_TILE_X + (lane & 15);
	const int py0 = ty * GSR_TILE_Y + (lane >> 4);
	const uint2 range = ranges[tile];
	const uint32_t len = range.y - range.x;
	if (len == 0u) return;
	const uint32_t* plist = point_list + range.x;

	uint32_t pos[GSR_PIX_PER_LANE];   // the pixel's median position; GSR_MEDIAN_NONE: none, outside the image, or already summed
	float g[GSR_PIX_PER_LANE];
#pragma unroll
	for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
		const int py = py0 + 4 * k;
		const bool inside = px < W && py < H;
		const size_t pix_id = inside ? (size_t)W * py + px : 0;
		pos[k] = inside ? state[pix_id] : GSR_MEDIAN_NONE;
		g[k] = inside ? dL_dmedian[pix_id] : 0.f;
	}

	int cnt = 0;   // wave-uniform; at most 256: every round retires at least one of the 256 pixels
	for (;;) {
		// the next position: that of the lowest lane's lowest pixel still waiting
		const uint32_t cur = pos[0] != GSR_MEDIAN_NONE ? pos[0] : pos[1] != GSR_MEDIAN_NONE ? pos[1] : pos[2] != GSR_MEDIAN_NONE ? pos[2] : pos[3];
		const unsigned long long waiting = __builtin_amdgcn_ballot_w64(cur != GSR_MEDIAN_NONE);
		if (waiting == 0ull) break;   // wave-uniform
		const uint32_t q = (uint32_t)__builtin_amdgcn_readlane((int)cur, __builtin_ctzll(waiting));
		// the lane's pixels in the order k = 0..3, then the lanes by a xor butterfly: a fixed order, and every lane ends with the same
		// bits (an addition commutes bit for bit)
		float t = 0.f;
#pragma unroll
		for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
			const bool mine = pos[k] == q;
			t += mine ? g[k] : 0.f;
			pos[k] = mine ? GSR_MEDIAN_NONE : pos[k];
		}
#pragma unroll
		for (int off = 1; off < 64; off <<= 1) t += __shfl_xor(t, off, 64);
		if (lane == 0) { sq[cnt] = q; stot[cnt] = t; }
		cnt++;
	}
	__builtin_amdgcn_wave_barrier();   // a wave's LDS operations execute in program order; this keeps the compiler from moving them

	for (int e = lane; e < cnt; e += 64) {
		const uint32_t q = sq[e];
		if (q >= len) continue;   // the state is the caller's buffer: a plane that is not this view's must not index past the list
		const uint32_t id = plist[q];
		const uint2 r = reinterpret_cast<const uint2*>(splat + id)[3];   // rect_min, rect_wh
		const uint32_t slot = gsr_slot_index(slot_base[id], r.x, r.y, tx, ty);
		float* w = reinterpret_cast<float*>(slots + slot) + 9;   // pad0, the blend's own dL/dv
		*w = *w + stot[e];
	}
}

void gsr_launch_median_forward(const GsrFrame& f, float* out_depth, int32_t* out_median, int32_t* out_dominant, float* out_weight,
                               uint32_t* state, bool full_walk)
{
	const GsrTileGrid t = gsr_tile_grid(f.W, f.H);
	if (full_walk)
		gsr_launch(gsr_median_forward_kernel<false>, t.grid, t.block, 0, f.s, nullptr, nullptr, f.W, f.H, t.gx, t.ntiles, f.img.ranges, f.bin.point_list,
		           f.g.splat, f.img.n_contrib, f.img.tile_max_contrib, out_depth, out_median, out_dominant, out_weight, state, f.cull ? 1 : 0);
	else
		gsr_launch(gsr_median_forward_kernel<true>, t.grid, t.block, 0, f.s, nullptr, nullptr, f.W, f.H, t.gx, t.ntiles, f.img.ranges, f.bin.point_list,
		           f.g.splat, f.img.n_contrib, f.img.tile_max_contrib, out_depth, out_median, out_dominant, out_weight, state, f.cull ? 1 : 0);
}

void gsr_launch_median_backward(const GsrFrame& f, const uint32_t* state, const float* dL_dmedian)
{
	const GsrTileGrid t = gsr_tile_grid(f.W, f.H);
	gsr_launch(gsr_median_backward_kernel, t.grid, t.block, 0, f.s, nullptr, nullptr, f.W, f.H, t.gx, t.ntiles,
	           f.img.ranges, f.bin.point_list, f.g.splat, f.g.slot_base, state, dL_dmedian, f.slots);
}
