// contrib.hip -- per-Gaussian blend-weight statistics of one view (include/gsr_contrib.h): for every Gaussian g the sum over the pixels
// of m(p) w_g(p), the maximum of w_g(p) and the number of pixels it blended into, with w = alpha * T the weight the forward blend
// multiplied the colour by.  Two kernels, no atomics, no workgroup barrier, bitwise reproducible.
//
// Tile pass: the replay walk (gsr_replay.h), front to back, with the slot address.  Nothing of the state is written (not tile_order,
// not the backward's validity bytes), so the pass may run before or after the backward of the same forward.
//
// Per instance with at least one hit each lane holds two partials over its four pixels (sum of m w, max of w); the hit count is a
// scalar -- the hit tests are lane masks already, four s_bcnt1 add them up.  The wave reduction of the two partials is deferred the way
// the backward's flush defers its own (render_backward.hip GSR_BWD_FLUSH): a lane parks its two partials in LDS (one ds_write2_b32 per
// reduced instance, and lane 0 a ds_write_b64 with the slot and the count), and once GSR_CONTRIB_FLUSH instances wait they are finished
// together -- lane (instance i, value v, quarter q) reads 16 of the 64 partials of row (i, v) with four ds_read_b128, folds them (every
// lane forms the 16-way sum and the 16-way max and keeps its own), and three lane exchanges (ds_bpermute_b32: the LDS pipe, not DPP)
// join the quarters and bring the max beside the sum.  In the gfx950 ISA a flush of eight is 4 ds_read_b128, about 45 VALU, 3
// ds_bpermute_b32 and a ds_read_b64 before the stores: with the parking, 6 to 8 vector or LDS instructions per reduced instance
// against the 12 DPP moves and 12 adds / maxes of reducing each instance on its own.  The result goes, with plain stores, into the instance's
// own 16-byte record {sum, max, count, 1}: the slot numbering of the backward's gradient slots (gsr_slot_index), and its validity
// byte is set.
//
// Validity: slots of tiles the trim words left out, and of instances without a hit, are never written.  The caller's scratch may be
// uninitialised: the call clears the validity bytes (one byte per slot, behind the records) on the stream before the tile pass, and
// the per-Gaussian pass trusts those bytes alone -- the fourth word of a record only pads it to one 16-byte store.
//
// Per-Gaussian pass: one lane per Gaussian folds the slots [slot_base[g], slot_base[g] + tiles_touched[g]) in index order and updates
// the outputs in place (sum +=, max = max, count +=); a Gaussian without a valid slot is left untouched (the stat_* convention of the
// backward, gsr.h), so a sweep over views accumulates without further launches.
#include "gsr_replay.h"

#define GSR_CONTRIB_FLUSH 8   // reduced instances finished together: 8 x 2 rows x 4 quarters = 64 lanes

struct __attribute__((aligned(16))) GsrContribSlot {
	float sum, max;
	uint32_t count, one;
};
static_assert(sizeof(GsrContribSlot) == 16, "contribution record must be 16 bytes");

struct GsrContribPass : GsrReplayPass {
	struct Acc {
		float s, mx;     // the lane's sum of m w and max of w over its four pixels
		uint32_t hits;   // wave-uniform
	};
	float mw[GSR_PIX_PER_LANE];
	// parked partials: row 2 i + v holds the 64 lanes' value v (0: sum, 1: max) of pending instance i; meta: its slot and hit count
	float* pend;
	uint2* meta;
	GsrContribSlot* __restrict__ slots;
	uint8_t* __restrict__ slot_valid;
	int npend;   // wave-uniform: reduced instances waiting in pend

	__device__ __forceinline__ Acc begin(const GsrInstance&) const { return Acc{0.f, 0.f, 0u}; }
	__device__ __forceinline__ void pixel(const GsrTileWalk&, const GsrInstance&, int k, float, const GsrPairFwd& p, Acc& a) const
	{
		a.hits += (uint32_t)__popcll(p.hitm);
		a.s = __builtin_fmaf(mw[k], p.w, a.s);
		a.mx = fmaxf(a.mx, p.w);
	}
	__device__ __forceinline__ void finish(const GsrTileWalk& w, const GsrInstance& in, Acc& a)
	{
		if (a.hits == 0u) return;   // wave-uniform: no record for an instance without a hit
		pend[(2 * npend) * GSR_REPLAY_ROW + w.lane] = a.s;
		pend[(2 * npend + 1) * GSR_REPLAY_ROW + w.lane] = a.mx;
		if (w.lane == 0) meta[npend] = make_uint2(in.slot(), a.hits);
		if (++npend == GSR_CONTRIB_FLUSH) flush(w.lane);
	}
	// the flush: finishes the pending instances.  lane = 8 i + 4 v + q reads the partials of lanes 4 (q + 4 e) .. + 3, e = 0..3, of row
	// (i, v) and folds them in that order; the quarters are joined over lanes q ^ 1, q ^ 2, and value 0's lanes fetch the max from v = 1.
	// A wave's LDS operations execute in program order: the reads see every parked partial, the next stores come after them.
	__device__ __forceinline__ void flush(int lane)
	{
		__builtin_amdgcn_wave_barrier();
		const float* pr = pend + (lane >> 2) * GSR_REPLAY_ROW + 4 * (lane & 3);
		const float4 q0 = *reinterpret_cast<const float4*>(pr), q1 = *reinterpret_cast<const float4*>(pr + 16);
		const float4 q2 = *reinterpret_cast<const float4*>(pr + 32), q3 = *reinterpret_cast<const float4*>(pr + 48);
		const bool is_max = (lane & 4) != 0;
		const float ts = (((q0.x + q0.y) + (q0.z + q0.w)) + ((q1.x + q1.y) + (q1.z + q1.w))) + (((q2.x + q2.y) + (q2.z + q2.w)) + ((q3.x + q3.y) + (q3.z + q3.w)));
		const float tm = fmaxf(fmaxf(fmaxf(fmaxf(q0.x, q0.y), fmaxf(q0.z, q0.w)), fmaxf(fmaxf(q1.x, q1.y), fmaxf(q1.z, q1.w))),
		                       fmaxf(fmaxf(fmaxf(q2.x, q2.y), fmaxf(q2.z, q2.w)), fmaxf(fmaxf(q3.x, q3.y), fmaxf(q3.z, q3.w))));
		float t = is_max ? tm : ts;
		float o = __shfl_xor(t, 1, 64);
		t = is_max ? fmaxf(t, o) : t + o;
		o = __shfl_xor(t, 2, 64);
		t = is_max ? fmaxf(t, o) : t + o;
		const float mx = __shfl_xor(t, 4, 64);
		const int inst = lane >> 3;
		if ((lane & 7) == 0 && inst < npend) {
			const uint2 m = meta[inst];
			GsrContribSlot r;
			r.sum = t; r.max = mx; r.count = m.y; r.one = 1u;
			slots[m.x] = r;
			slot_valid[m.x] = 1;
		}
		npend = 0;
		__builtin_amdgcn_wave_barrier();
	}
};

// declared for six waves per SIMD (80 VGPRs): left to itself the allocator takes 82 and gives one away
__global__ void __launch_bounds__(64 * GSR_WAVES_PER_WG) __attribute__((amdgpu_waves_per_eu(6))) gsr_contrib_tiles_kernel(
	int W, int H, int gx, int ntiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
	const GsrSplat* __restrict__ splat, const uint32_t* __restrict__ slot_base, const uint32_t* __restrict__ n_contrib,
	const uint32_t* __restrict__ tile_max_contrib, const float* __restrict__ pixel_weight, GsrContribSlot* __restrict__ slots,
	uint8_t* __restrict__ slot_valid, int cull)
{
	__shared__ GsrBatchLds s_batch[GSR_WAVES_PER_WG];
	__shared__ __attribute__((aligned(16))) float s_pend[GSR_WAVES_PER_WG][2 * GSR_CONTRIB_FLUSH * GSR_REPLAY_ROW];
	__shared__ uint2 s_meta[GSR_WAVES_PER_WG][GSR_CONTRIB_FLUSH];
	GsrTileWalk w;
	gsr_walk_tile(w, gx);
	if (w.tile >= ntiles) return;
	gsr_walk_list(w, ranges, point_list, tile_max_contrib);
	if (w.n <= 0) return;
	GsrContribPass pass;
	gsr_walk_pixels<uint32_t>(w, W, H, n_contrib, nullptr,
	                          [&](int k, bool inside, uint32_t pix_id) { pass.mw[k] = (inside && pixel_weight) ? pixel_weight[pix_id] : 1.0f; });
	pass.pend = s_pend[w.wave];
	pass.meta = s_meta[w.wave];
	pass.slots = slots;
	pass.slot_valid = slot_valid;
	pass.npend = 0;
	GSR_REPLAY(false, true, w, s_batch[w.wave], splat, slot_base, cull, pass);
	if (pass.npend) pass.flush(w.lane);
}

// one lane per Gaussian; four validity bytes, then their records, are requested together
__global__ void __launch_bounds__(256) gsr_contrib_gaussians_kernel(int P, const uint32_t* __restrict__ tiles_touched, const uint32_t* __restrict__ slot_base,
                                                                    const GsrContribSlot* __restrict__ slots, const uint8_t* __restrict__ slot_valid,
                                                                    float* __restrict__ weight_sum, float* __restrict__ weight_max,
                                                                    int32_t* __restrict__ pixel_count)
{
	const int g = blockIdx.x * 256 + threadIdx.x;
	if (g >= P) return;
	const uint32_t tiles = tiles_touched[g];
	if (tiles == 0u) return;   // culled: slot_base was never written
	const uint32_t base = slot_base[g];
	float s = 0.f, mx = 0.f;
	uint32_t c = 0u;
	bool any = false;
	for (uint32_t k = 0; k < tiles; k += 4) {
		uint8_t v[4];
		GsrContribSlot r[4];
#pragma unroll
		for (int i = 0; i < 4; i++) v[i] = (k + i < tiles) ? slot_valid[base + k + i] : (uint8_t)0;
#pragma unroll
		for (int i = 0; i < 4; i++)
			if (v[i]) r[i] = slots[base + k + i];
#pragma unroll
		for (int i = 0; i < 4; i++)
			if (v[i]) { s += r[i].sum; mx = fmaxf(mx, r[i].max); c += r[i].count; any = true; }
	}
	if (!any) return;
	if (weight_sum) weight_sum[g] += s;
	if (weight_max) weight_max[g] = fmaxf(weight_max[g], mx);
	if (pixel_count) pixel_count[g] += (int32_t)c;
}

size_t gsr_contrib_valid_offset(int64_t R) { return gsr_align_up((size_t)R * sizeof(GsrContribSlot)); }

void gsr_launch_contrib_tiles(const GsrFrame& f, const float* pixel_weight, void* scratch)
{
	const GsrTileGrid t = gsr_tile_grid(f.W, f.H);
	uint8_t* valid = (uint8_t*)scratch + gsr_contrib_valid_offset(f.R);
	gsr_launch(gsr_contrib_tiles_kernel, t.grid, t.block, 0, f.s, nullptr, nullptr, f.W, f.H, t.gx, t.ntiles, f.img.ranges, f.bin.point_list, f.g.splat,
	           f.g.slot_base, f.img.n_contrib, f.img.tile_max_contrib, pixel_weight, (GsrContribSlot*)scratch, valid, f.cull ? 1 : 0);
}

void gsr_launch_contrib_gaussians(const GsrFrame& f, const void* scratch, float* weight_sum, float* weight_max, int32_t* pixel_count)
{
	gsr_launch(gsr_contrib_gaussians_kernel, dim3((f.P + 255) / 256), dim3(256), 0, f.s, nullptr, nullptr, f.P, f.g.tiles_touched, f.g.slot_base,
	           (const GsrContribSlot*)scratch, (const uint8_t*)scratch + gsr_contrib_valid_offset(f.R), weight_sum, weight_max, pixel_count);
}
