// absgrad.hip -- per-Gaussian fold of the absolute screen-space gradients (include/gsr_absgrad.h).
//
// The ABS variant of the backward blend (render_backward.hip) leaves, in words 10 and 11 of every valid (Gaussian, tile) gradient
// slot, that tile's sums over its pixels of |d L_p / d mean2D.x| and |d L_p / d mean2D.y| -- the moduli taken per pixel, before any
// sum, already in the units of dL/dmean2D (0.5 W, 0.5 H).  Here one lane per Gaussian adds the two words of its run of slots
// [slot_base[g], slot_base[g] + tiles_touched[g]) in ascending slot order, four slots per round (their validity bytes are requested
// together, then the records of the valid ones); runs of more than GSR_SLOT_COOP slots are added by the whole wave, lanes striding
// over the run, and reduced with DPP, as the per-Gaussian backward adds the other words of such runs (gaussian_backward.hip
// gsr_add_slot).  The order depends on the launch geometry alone: no atomics, the same bits in every run.
//
// Every Gaussian of the range gets its pair written -- exact zeros when it is culled or owns no valid slot -- so the output needs
// no initialisation; the accumulator of the densification statistic is touched for visible Gaussians only (radii > 0, the rule of the
// stat_* arrays of gsr_backward_args).  A pass of its own on purpose: gsr_gaussian_backward_kernel and its instantiations stay as
// they are; the extra read is one validity byte and eight bytes per slot.
#include "gsr_internal.h"

#define GSR_ABS_THREADS 64   // one wave per workgroup: the cooperative runs need no workgroup barrier
#define GSR_ABS_ROUND 4      // slots requested per round of the per-lane sum

// words 10 and 11 of slot s (byte 40 of a 48-byte record: 8-byte aligned)
__device__ __forceinline__ float2 gsr_abs_words(const GsrGradSlot* __restrict__ slots, uint32_t s)
{
	return *reinterpret_cast<const float2*>(&slots[s].pad1);
}

__global__ void __launch_bounds__(GSR_ABS_THREADS) gsr_absgrad_fold_kernel(
	int first, int count, const uint32_t* __restrict__ tiles_touched, const uint32_t* __restrict__ slot_base, const int* __restrict__ radii,
	const GsrGradSlot* __restrict__ slots, const uint8_t* __restrict__ slot_valid, float* __restrict__ abs_dL_dmean2D,
	float* __restrict__ stat_abs_gradient_accum)
{
	const int lane = threadIdx.x & 63;
	const int idx = first + blockIdx.x * GSR_ABS_THREADS + threadIdx.x;
	const bool in_range = idx < first + count;
	uint32_t tiles = 0, base = 0;
	bool visible = false;
	if (in_range) {
		tiles = tiles_touched[idx];
		// radii > 0 <=> tiles_touched > 0 (the forward zeroes both together; culled: slot_base was never written)
		visible = radii ? radii[idx] > 0 : tiles > 0;
		if (!visible || !slot_valid) tiles = 0;
		if (tiles) base = slot_base[idx];
	}
	float ax = 0.f, ay = 0.f;
	if (tiles <= GSR_SLOT_COOP) {
		for (uint32_t k = 0; k < tiles; k += GSR_ABS_ROUND) {
			uint8_t v[GSR_ABS_ROUND];
			float2 r[GSR_ABS_ROUND];
#pragma unroll
			for (int i = 0; i < GSR_ABS_ROUND; i++) v[i] = (k + i < tiles) ? slot_valid[base + k + i] : (uint8_t)0;
#pragma unroll
			for (int i = 0; i < GSR_ABS_ROUND; i++)
				if (v[i]) r[i] = gsr_abs_words(slots, base + k + i);
#pragma unroll
			for (int i = 0; i < GSR_ABS_ROUND; i++)
				if (v[i]) { ax += r[i].x; ay += r[i].y; }
		}
	}
	unsigned long long big = __builtin_amdgcn_ballot_w64(tiles > GSR_SLOT_COOP);
	while (big) {  // wave-uniform
		const int src = __ffsll((long long)big) - 1;
		big &= big - 1;
		const uint32_t s_tiles = __shfl(tiles, src, 64), s_base = __shfl(base, src, 64);
		float px = 0.f, py = 0.f;
		for (uint32_t k = lane; k < s_tiles; k += 64)
			if (slot_valid[s_base + k]) {
				const float2 w = gsr_abs_words(slots, s_base + k);
				px += w.x; py += w.y;
			}
		const float tx = __shfl(gsr_wave_sum_to_lane63(px), 63, 64), ty = __shfl(gsr_wave_sum_to_lane63(py), 63, 64);
		if (lane == src) { ax = tx; ay = ty; }
	}
	if (!in_range) return;
	if (abs_dL_dmean2D) {   // (two dword stores: the caller's array need not be 8-byte aligned)
		abs_dL_dmean2D[2 * (size_t)idx] = ax;
		abs_dL_dmean2D[2 * (size_t)idx + 1] = ay;
	}
	if (stat_abs_gradient_accum && visible) stat_abs_gradient_accum[idx] += hypotf(ax, ay);   // (no underflow of the squares: a barely visible Gaussian's sums are tiny)
}

void gsr_launch_absgrad_fold(const GsrFrame& f, int first, int count, const int* radii, float* abs_dL_dmean2D, float* stat_abs_gradient_accum)
{
	gsr_launch(gsr_absgrad_fold_kernel, dim3((count + GSR_ABS_THREADS - 1) / GSR_ABS_THREADS), dim3(GSR_ABS_THREADS), 0, f.s, nullptr, nullptr,
	           first, count, f.g.tiles_touched, f.g.slot_base, radii, f.slots, f.slot_valid, abs_dL_dmean2D, stat_abs_gradient_accum);
}
