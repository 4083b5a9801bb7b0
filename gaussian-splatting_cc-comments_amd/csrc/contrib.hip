// contrib.hip -- per-Gaussian blend-weight statistics of one view (include/gsr_contrib.h): for every Gaussian g the sum over the pixels
// of m(p) w_g(p), the maximum of w_g(p) and the number of pixels it blended into, with w = alpha * T the weight the forward blend
// multiplied the colour by.  Two kernels, no atomics, no workgroup barrier, bitwise reproducible.
//
// Tile pass: the forward's walk over again (render_forward.hip) -- one wave64 per 16x16 tile, four pixels per lane, 64 instances
// staged per batch into the wave's LDS slice behind gsr_tile_band_mask -- but from the state the forward left: the list positions
// [0, min(range length, tile_max_contrib)), and for a pixel only the positions in front of its n_contrib.  `power`, alpha, the two
// thresholds and T's update are the forward's own instruction sequence on the same records, so every w has the forward's bits and no
// accept / reject decision differs.  Nothing of the state is written (not tile_order, not the backward's validity bytes), so the pass
// may run before or after the backward of the same forward.  tile_order is not read either: tiles are taken in index order.
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
// own 16-byte record {sum, max, count, 1}: slot = slot_base[id] + (ty - rect_min.y) * rect_w + (tx - rect_min.x), the numbering of
// the backward's gradient slots (render_backward.hip), and its validity byte is set.
//
// Validity: slots of tiles the trim words left out, and of instances without a hit, are never written.  The caller's scratch may be
// uninitialised: the call clears the validity bytes (one byte per slot, behind the records) on the stream before the tile pass, and
// the per-Gaussian pass trusts those bytes alone -- the fourth word of a record only pads it to one 16-byte store.
//
// Per-Gaussian pass: one lane per Gaussian folds the slots [slot_base[g], slot_base[g] + tiles_touched[g]) in index order and updates
// the outputs in place (sum +=, max = max, count +=); a Gaussian without a valid slot is left untouched (the stat_* convention of the
// backward, gsr.h), so a sweep over views accumulates without further launches.
#include "render_common.h"

#define GSR_CONTRIB_FLUSH 8   // reduced instances finished together: 8 x 2 rows x 4 quarters = 64 lanes
#define GSR_CONTRIB_ROW 80    // words between two rows of parked partials: the two rows of an 8-lane read group then sit 16 banks apart

struct __attribute__((aligned(16))) GsrContribSlot {
	float sum, max;
	uint32_t count, one;
};
static_assert(sizeof(GsrContribSlot) == 16, "contribution record must be 16 bytes");

__global__ void __launch_bounds__(64 * GSR_WAVES_PER_WG) gsr_contrib_tiles_kernel(
	int W, int H, int gx, int ntiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
	const GsrSplat* __restrict__ splat, const uint32_t* __restrict__ slot_base, const uint32_t* __restrict__ n_contrib,
	const uint32_t* __restrict__ tile_max_contrib, const float* __restrict__ pixel_weight, GsrContribSlot* __restrict__ slots,
	uint8_t* __restrict__ slot_valid, int cull)
{
	// the surviving instances of a batch: (x, y, -0.5 conic a, conic b), (-0.5 conic c, opacity, list position, slot), band mask
	__shared__ float4 s_rec[GSR_WAVES_PER_WG][2][64];
	__shared__ uint32_t s_bands[GSR_WAVES_PER_WG][64];
	// parked partials: row 2 i + v holds the 64 lanes' value v (0: sum, 1: max) of pending instance i; s_meta: its slot and hit count
	__shared__ __attribute__((aligned(16))) float s_pend[GSR_WAVES_PER_WG][2 * GSR_CONTRIB_FLUSH * GSR_CONTRIB_ROW];
	__shared__ uint2 s_meta[GSR_WAVES_PER_WG][GSR_CONTRIB_FLUSH];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int tile = blockIdx.x * GSR_WAVES_PER_WG + wave;
	if (tile >= ntiles) return;  // wave-uniform; no barriers below
	float4(*rec)[64] = s_rec[wave];
	uint32_t* recb = s_bands[wave];
	float* pend = s_pend[wave];
	uint2* meta = s_meta[wave];

	const int tx = tile % gx, ty = tile / gx;
	const int px = tx * GSR_TILE_X + (lane & 15);
	const int py0 = ty * GSR_TILE_Y + (lane >> 4);
	const float pfx = (float)px;
	const float x0f = (float)(tx * GSR_TILE_X), y0f = (float)(ty * GSR_TILE_Y);

	const uint2 range = ranges[tile];
	const int n = (int)min(range.y - range.x, tile_max_contrib[tile]);  // the tail was never blended
	if (n <= 0) return;
	const uint32_t* plist = point_list + range.x;

	float T[GSR_PIX_PER_LANE], mw[GSR_PIX_PER_LANE], pfy[GSR_PIX_PER_LANE];
	uint32_t last[GSR_PIX_PER_LANE];   // the pixel's n_contrib: it blended positions in front of this one only (0 outside the image)
	uint32_t band_last[GSR_PIX_PER_LANE];   // wave-uniform: the largest of them in band k
#pragma unroll
	for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
		const int py = py0 + 4 * k;
		const bool inside = px < W && py < H;
		const uint32_t pix_id = inside ? (uint32_t)(W * py + px) : 0u;
		pfy[k] = (float)py;
		T[k] = 1.0f;
		last[k] = inside ? n_contrib[pix_id] : 0u;
		mw[k] = (inside && pixel_weight) ? pixel_weight[pix_id] : 1.0f;
		uint32_t m = last[k];
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
		band_last[k] = __builtin_amdgcn_readfirstlane(m);
	}

	// software pipeline: records one batch ahead, ids two batches ahead
	float4 ra = make_float4(0, 0, 0, 0), rb = ra;
	uint32_t sbase = 0u;
	if (lane < n) {
		const uint32_t id = plist[lane];
		const float4* p = reinterpret_cast<const float4*>(splat + id);
		ra = p[0]; rb = p[1];
		sbase = slot_base[id];
	}
	uint32_t id_next = (64 + lane < n) ? plist[64 + lane] : 0u;
	int npend = 0;   // wave-uniform: reduced instances waiting in s_pend

	// the flush: finishes the pending instances.  lane = 8 i + 4 v + q reads the partials of lanes 4 (q + 4 e) .. + 3, e = 0..3, of row
	// (i, v) and folds them in that order; the quarters are joined over lanes q ^ 1, q ^ 2, and value 0's lanes fetch the max from v = 1.
	// A wave's LDS operations execute in program order: the reads see every parked partial, the next stores come after them.
	auto flush = [&]() {
		__builtin_amdgcn_wave_barrier();
		const float* pr = pend + (lane >> 2) * GSR_CONTRIB_ROW + 4 * (lane & 3);
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
	};

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
			rec[1][pos] = make_float4(-0.5f * rb.x, rb.y, __uint_as_float((uint32_t)(base + lane)), __uint_as_float(slot));
			recb[pos] = bands;
		}
		if (base + 64 + lane < n) {
			const float4* p = reinterpret_cast<const float4*>(splat + id_next);
			ra = p[0]; rb = p[1];
			sbase = slot_base[id_next];
		}
		id_next = (base + 128 + lane < n) ? plist[base + 128 + lane] : 0u;
		__builtin_amdgcn_wave_barrier();

		for (int j = 0; j < cnt; j++) {
			const float4 A = rec[0][j];   // x, y, -0.5 conic a, conic b
			const float4 B = rec[1][j];   // -0.5 conic c, opacity, list position, slot
			const uint32_t position = __builtin_amdgcn_readfirstlane(__float_as_uint(B.z));   // wave-uniform
			const uint32_t jbands = __builtin_amdgcn_readfirstlane(recb[j]);                  // wave-uniform
			const float dx = A.x - pfx;
			const float ax2 = __fmul_rn(__fmul_rn(A.z, dx), dx), bdx = __fmul_rn(A.w, dx);
			float s = 0.f, mx = 0.f;
			uint32_t hits = 0u;   // wave-uniform
#pragma unroll
			for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
				if (!(jbands & (1u << k)) || position >= band_last[k]) continue;  // scalar branch: the band cannot be reached, or it had finished
				const float dy = A.y - pfy[k];
				const float power = gsr_pair_power_halved(ax2, bdx, B.x, dy);
				const float alpha = fminf(0.99f, B.y * __expf(power));
				const unsigned long long hitm = __builtin_amdgcn_ballot_w64(position < last[k]) & __builtin_amdgcn_ballot_w64(!(power > 0.0f)) &
				                                __builtin_amdgcn_ballot_w64(!(alpha < 1.0f / 255.0f));
				if (hitm == 0ull) continue;  // wave-uniform
				hits += (uint32_t)__popcll(hitm);
				const bool hit = __builtin_amdgcn_inverse_ballot_w64(hitm);
				const float w = hit ? __fmul_rn(alpha, T[k]) : 0.0f;                  // the forward's alpha * T
				T[k] = hit ? __fmul_rn(T[k], __fsub_rn(1.0f, alpha)) : T[k];          // ... and its T (1 - alpha), rounded as there
				s = __builtin_fmaf(mw[k], w, s);
				mx = fmaxf(mx, w);
			}
			if (hits == 0u) continue;   // wave-uniform: no record for an instance without a hit
			const uint32_t slot = __builtin_amdgcn_readfirstlane(__float_as_uint(B.w));
			pend[(2 * npend) * GSR_CONTRIB_ROW + lane] = s;
			pend[(2 * npend + 1) * GSR_CONTRIB_ROW + lane] = mx;
			if (lane == 0) meta[npend] = make_uint2(slot, hits);
			if (++npend == GSR_CONTRIB_FLUSH) flush();
		}
		__builtin_amdgcn_wave_barrier();
	}
	if (npend) flush();
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

void gsr_launch_contrib_tiles(int W, int H, GsrImage img, const uint32_t* point_list, const GsrSplat* splat, const uint32_t* slot_base,
                              const float* pixel_weight, void* scratch, int64_t R, bool cull, hipStream_t s)
{
	const int gx = gsr_grid_x(W), ntiles = gx * gsr_grid_y(H);
	uint8_t* valid = (uint8_t*)scratch + gsr_contrib_valid_offset(R);
	gsr_launch(gsr_contrib_tiles_kernel, dim3((ntiles + GSR_WAVES_PER_WG - 1) / GSR_WAVES_PER_WG), dim3(64 * GSR_WAVES_PER_WG), 0, s, nullptr, nullptr,
	           W, H, gx, ntiles, img.ranges, point_list, splat, slot_base, img.n_contrib, img.tile_max_contrib, pixel_weight,
	           (GsrContribSlot*)scratch, valid, cull ? 1 : 0);
}

void gsr_launch_contrib_gaussians(int P, GsrGeometry g, const void* scratch, int64_t R, float* weight_sum, float* weight_max, int32_t* pixel_count,
                                  hipStream_t s)
{
	gsr_launch(gsr_contrib_gaussians_kernel, dim3((P + 255) / 256), dim3(256), 0, s, nullptr, nullptr, P, g.tiles_touched, g.slot_base,
	           (const GsrContribSlot*)scratch, (const uint8_t*)scratch + gsr_contrib_valid_offset(R), weight_sum, weight_max, pixel_count);
}
