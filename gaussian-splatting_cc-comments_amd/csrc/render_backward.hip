// render_backward.hip -- per-tile back-to-front gradient of the alpha compositing.
//
// Replaces renderCUDA<3> backward (cuda_rasterizer/backward.cu:408-601).  The reference issues
// nine fp32 atomicAdd per contributing (pixel, Gaussian) pair, all 256 lanes of a tile hitting the
// same addresses -- the slowest atomic shape on this chip (MI355X_MICROARCH.md "Global float
// atomics").  Here one wave64 owns the tile (render_common.h): per surviving instance each lane
// first adds its four pixels' partials in registers -- six sums for the nine words: the five geometric words are moments of
// f = o g, g = G dL/dalpha, and neither the opacity o (one value per instance) nor dx (one value per lane: its four pixels share
// their column) varies over a lane's sum, so the lane keeps sum g, sum g dy, sum g dy^2 and the three colour sums, forms
// dx sum g, dx^2 sum g, dx sum g dy and the five products with o once per reduced instance ("per-lane partial sums" in the
// kernel; 8 issue slots per evaluated pair instead of 13, 8 more per reduction); the wave then folds the nine values through LDS --
// lane l stores eight of them as row l of a 64 x 9-word area (odd row stride: 64 rows, 64 banks), the
// eight lanes of group c add column c (eight rows each).  What is left -- the three DPP steps over
// each group's column sums, the ninth value's sum over the wave, the epilogue and the stores -- is
// done for four reduced instances at a time, by one instruction stream whose 64 lanes are the four
// instances' 8 values and 8 groups of the ninth (s_pend; the AUX variant finishes every instance on
// its own: a DPP chain for the ninth and tenth values under the LDS round trip, round 3; rounds 1-2
// used a v_permlane32/16_swap butterfly on the vector ALU, the port this kernel is bound by) -- and
// the tile's total for this (Gaussian, tile) instance is written once, with plain stores, into that instance's own 48-byte
// slot (slot = its position in the depth-ordered, per-Gaussian-contiguous emission order).  The
// per-Gaussian kernel then adds each Gaussian's contiguous run of slots in a fixed order: no
// atomics, no workgroup barrier (a wave's LDS operations execute in program order), bitwise
// reproducible.  Per-pixel arithmetic is that of backward.cu:507-599; G and alpha come
// from the same roundings as in the forward kernel (gsr_pair_power; the forward's pre-halved conic terms give the same
// bits), so the products the forward formed are the ones undone here.
//
// A lane's four pixels are two packed pairs: pair p holds the tile's band 2p (rows 8p .. 8p+3) in the .x halves of its v2f
// registers and band 2p+1 in the .y halves.  Per staged instance each pair has a wave-uniform mode, two bits that say which of its
// bands can be reached (gsr_tile_band_mask, as the forward blend evaluated and stored it: "The band masks" below) and still have an instance to come (the band's largest n_contrib lies behind this one):
//   0  the pair is skipped;
//   3  the packed body: every operation a v_pk_*_f32 on both halves;
//   1, 2  the same operations in the same order as plain fp32 instructions on the .x or the .y half alone.  The other band could
//         not have hit: its alpha would be forced to 0, its state update the identity bit for bit, its additions exact zeros --
//         leaving it out leaves the same sums (the sign of a zero in a per-lane partial aside, which the per-Gaussian pass,
//         adding every slot to 0.f, does not see).
// The modes are decided by the staging lanes; the body is written once over the mode (gsr_half below, the lambda `pair` in the kernel).  The default
// instantiation has all four modes; AUX and ABS have no registers for them and evaluate every pair that is not skipped whole.
// With GSR_DEBUG_NO_CULL every pair that has an instance left is evaluated whole by every instantiation.
#include "render_common.h"
#include <type_traits>

#define GSR_BWD_NV 9
#ifndef GSR_BWD_BAND_LAST
#define GSR_BWD_BAND_LAST 1   // 0 (A/B builds): a band is left out of a pair by the band mask alone, not by its largest n_contrib
#endif
#define GSR_BWD_FLUSH 4   // reduced instances finished together (default variant): 4 x (8 values + 8 groups of the ninth) = 64 lanes
typedef float v2f __attribute__((ext_vector_type(2)));

GSR_TILE_CLOCK_BUFFER(gsr_backward_tile_clock, gsr_debug_tile_clock_backward)

// x + y of a pixel pair as ONE v_add_f32 on the pair's two registers.  Left to itself the compiler packs two such sums into a
// v_pk_add_f32 and pays three v_mov_b32 to line the operands up (16 instructions for eight sums instead of 8).
__device__ __forceinline__ float gsr_add_halves(v2f a)
{
	float r;
	asm("v_add_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a.x), "v"(a.y));
	return r;
}

// The pair body (the lambda `pair` in the kernel) is written once over a "mode" M, the pair's two reachable-band bits: M = 3 works on both halves of
// every register pair (v2f: v_pk_*_f32), M = 1 on the .x half and M = 2 on the .y half alone (float: plain fp32 instructions that
// name that half of the pair as their register; the other half is neither read nor written).  gsr_half<M> is the value type with
// its access to a pair; the overloads below are the operations that have no common spelling for float and v2f.
template <int M> struct gsr_half;
template <> struct gsr_half<3> {
	typedef v2f type;
	static __device__ __forceinline__ v2f get(const v2f& a) { return a; }
	static __device__ __forceinline__ void set(v2f& d, v2f s) { d = s; }
	static __device__ __forceinline__ v2f select(bool h0, bool h1, v2f a) { return v2f{h0 ? a.x : 0.f, h1 ? a.y : 0.f}; }
};
template <> struct gsr_half<1> {
	typedef float type;
	static __device__ __forceinline__ float get(const v2f& a) { return a.x; }
	static __device__ __forceinline__ void set(v2f& d, float s) { d.x = s; }
	static __device__ __forceinline__ float select(bool h0, bool, float a) { return h0 ? a : 0.f; }
};
template <> struct gsr_half<2> {
	typedef float type;
	static __device__ __forceinline__ float get(const v2f& a) { return a.y; }
	static __device__ __forceinline__ void set(v2f& d, float s) { d.y = s; }
	static __device__ __forceinline__ float select(bool, bool h1, float a) { return h1 ? a : 0.f; }
};
__device__ __forceinline__ float gsr_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ v2f gsr_fma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float gsr_exp2(float a) { return __builtin_amdgcn_exp2f(a); }
__device__ __forceinline__ v2f gsr_exp2(v2f a) { return v2f{__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)}; }
__device__ __forceinline__ float gsr_rcp(float a) { return __builtin_amdgcn_rcpf(a); }
__device__ __forceinline__ v2f gsr_rcp(v2f a) { return v2f{__builtin_amdgcn_rcpf(a.x), __builtin_amdgcn_rcpf(a.y)}; }
__device__ __forceinline__ float gsr_min99(float a) { return fminf(0.99f, a); }
__device__ __forceinline__ v2f gsr_min99(v2f a) { return v2f{fminf(0.99f, a.x), fminf(0.99f, a.y)}; }
__device__ __forceinline__ float gsr_lo(float a) { return a; }   // the value of the first / the second band of the mode
__device__ __forceinline__ float gsr_lo(v2f a) { return a.x; }
__device__ __forceinline__ float gsr_hi(float a) { return a; }
__device__ __forceinline__ float gsr_hi(v2f a) { return a.y; }
__device__ __forceinline__ float gsr_abs_sum(float a) { return __builtin_fabsf(a); }
__device__ __forceinline__ float gsr_abs_sum(v2f a) { return __builtin_fabsf(a.x) + __builtin_fabsf(a.y); }

// AUX (the depth-and-alpha variant, include/gsr.h gsr_aux_args): the depth channel is a fourth colour channel with background 0 --
// its accum_rec (restarted from ckpt_depth / final_D by the depth segments), (v - accum_rec_D) dL/dD in dL/dalpha -- dL/dA enters
// through the background term (A = 1 - T_final: -T_final (bg . dL/dpix - dL/dA)), and dL/dv = sum alpha T dL/dD is a tenth reduced
// partial, written to the slot's pad0.  Same slots, same order, no atomics.
// ABS (absolute screen-space gradients, include/gsr_absgrad.h): beside the signed sums every evaluated pair adds
// the moduli of its two per-pixel terms of dL/dmean2D, |f (a dx + b dy)| and |f (c dy + b dx)| -- taken per pixel, before any sum,
// so this variant alone still forms f = (o dL/dalpha) G, f dx and f dy per pixel, for the moduli only --
// into two more partials; both are reduced over the wave like the AUX variant's tenth value and written, scaled by 0.5 W / 0.5 H, to
// the slot's pad1 / pad2 (gsr_absgrad_fold_kernel, absgrad.hip, adds them per Gaussian).  The ABS instantiations finish every instance
// on its own, as the AUX ones do; the other nine (ten) words are computed by the same operations as without ABS.
// Waves per SIMD: four (at most 128 VGPRs) for every instantiation but <AUX, ABS>.  The AUX variant alone fills the 128 (left
// to itself the compiler takes 130), and the two accumulators, the halved b and the terms' temporaries of ABS on top spill 10
// registers to scratch at that limit: that instantiation takes 146 VGPRs (144 before the pair modes' staging) and runs three waves per
// SIMD, without scratch.  (Those are the counts with nine accumulators.  With six: default 122, ABS 118, AUX 124, <AUX, ABS> 130 VGPRs,
// the GSR_DEBUG_RECOMPUTE_BANDS twins 128 / 128 / 128 / 140; the same waves per SIMD, no scratch -- profiles/ab_c3_backward_moments.txt.)
//
// The band masks (RECOMPUTE = false, the product's kernels).  reach -- gsr_tile_band_mask of the record against this tile -- is the value
// the forward blend computed for the same list position from the same six record fields and the same tile origin, and stored as that
// position's byte of band_masks (render_forward.hip).  The byte is loaded with the position's id, at the same index (band_masks is
// indexed like point_list) and the same distance ahead; the record and the slot_base word of a position whose byte is 0 are not
// gathered (it is not staged: reach = 0), and gsr_tile_band_mask is not evaluated here.  Invariants:
//   * No byte is read that the forward did not write.  The walk ends at n = min(range length, tile_max_contrib).  tile_max_contrib is
//     a position (+ 1) inside a batch that some forward wave of the tile staged whole, and that wave stored the bytes of that batch and
//     of every batch before it.  For a band-split tile the maximum is taken over its four band waves and the argument holds for the wave
//     that has it.  A depth-segment wave here reads positions [seg_a, top) with top <= n.
//   * The load is in bounds wherever the id load beside it is: same index, one byte for four.
//   * cull == 0 (GSR_DEBUG_NO_CULL here) does not consult the array: reach = 0xF, every record gathered.  A forward run with
//     GSR_DEBUG_NO_CULL stored 0xF everywhere, which is what a default backward then reads.
//   * The bytes belong to the forward state: nothing after the forward blend writes them, so a second backward over the same state,
//     or over a state restored from a debug snapshot of the blobs, sees the same bytes.
// RECOMPUTE = true (GSR_DEBUG_RECOMPUTE_BANDS, kernels of their own): the array is ignored, every record of the walk is gathered and
// its mask computed from it.  Both forms stage the same instances with the same bands: the results are the same bits.
template <bool AUX, bool ABS, bool RECOMPUTE>
__device__ __forceinline__ void gsr_render_backward_wave(
	int W, int H, int gx, int nslots, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
	const uint8_t* __restrict__ band_masks, const GsrSplat* __restrict__ splat, const float4* __restrict__ checkpoints, const float* __restrict__ final_C, const uint32_t* __restrict__ slot_base, const float* __restrict__ bg,
	const float* __restrict__ final_Ts, const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max_contrib,
	const uint32_t* __restrict__ tile_order, const float* __restrict__ dL_dpixels, GsrGradSlot* __restrict__ slots,
	uint8_t* __restrict__ slot_valid, int cull, GsrAuxBlend aux)
{
	// per-wave staging of the surviving instances of a batch.  Every per-instance scalar that meets the
	// float2 pixel pairs is stored TWICE, so a ds_read_b128 delivers it as an aligned register pair ready
	// for v_pk_*_f32 (the compiler otherwise spends one v_mov per scalar per instance on the duplication).
	// (ROCm 7.2's compiler does fold a splat into op_sel / op_sel_hi for most packed operands by now; re-measured in round 3
	// with every scalar stored once -- three ds_read_b128 per instance instead of five and a dword, 119 VGPRs: 0.467 ->
	// 0.476 ms at C3, 1.616 -> 1.633 at C5, results identical.  The duplicated layout stays.)
	__shared__ float4 s_rec[GSR_WAVES_PER_WG][AUX ? 6 : 5][64];   // AUX: rec[5] = (v, v, -, -)
	__shared__ uint32_t s_bands[GSR_WAVES_PER_WG][64];
	// transposition area of the per-instance wave reduction: lane l stores its eight partials at row l (row stride 9 words:
	// 9 is odd, so the 64 rows of one store instruction fall into 64 different banks), then the eight lanes of group c read
	// column c, eight rows each
	__shared__ float s_red[GSR_WAVES_PER_WG][64 * 9 + 8];
	// deferred finish (default variant): per reduced instance, its 64 column sums (lane (g, r) of the transposition at g * 8 + r)
	// and the 64 lanes' v[8] (at 64 + lane); up to GSR_BWD_FLUSH instances wait here and are finished together (gsr_flush below).
	// 2 KB more per wave: 9.5 KB x 16 waves still fits one CU's 160 KB at 4 waves per SIMD.  The AUX variant keeps the
	// per-instance finish (its tenth value would leave fewer lanes per flush and its LDS would not fit 16 waves).
	__shared__ __attribute__((aligned(16))) float s_pend[GSR_WAVES_PER_WG][(AUX || ABS) ? 4 : GSR_BWD_FLUSH * 128];
	// the one-band pair modes (gsr_half): the default instantiation has the registers for them; AUX and ABS are full at their limits
	// with the packed body alone (spill 28 / 10 registers, <AUX, ABS> 158 VGPRs, with the three modes) and keep evaluating whole pairs
	constexpr bool ONE_BAND = !(AUX || ABS);
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int slot_id = blockIdx.x * GSR_WAVES_PER_WG + wave;
	if (slot_id >= nslots) return;  // wave-uniform; no barriers below
	GSR_TILE_CLOCK_START();
	GSR_TILE_STAT(unsigned long long st_staged = 0; unsigned long long st_pairs = 0; unsigned long long st_pairs_hit = 0; unsigned long long st_reductions = 0; unsigned long long st_lanes_hit = 0;
	              unsigned long long st_one_mask = 0; unsigned long long st_one_last = 0;)   // pairs evaluated on one band: by the band mask, by band_last
	// workgroups are dispatched in index order: tile_order lists the tiles by descending work, so the long tiles
	// start first and the short ones fill the end of the launch (binning.hip gsr_tile_order_kernel)
	// A heavy tile (walk of at least two checkpoint strides) comes as one entry per DEPTH SEGMENT (bits 28..31 = segment + 1):
	// this wave then walks the positions [a, b) of the list only, starting from the per-pixel (T, C) the forward left at b.
	const uint32_t entry = __builtin_amdgcn_readfirstlane(tile_order[slot_id]);
	if (entry == 0xFFFFFFFFu) return;  // unused segment entry
	const int tile = (int)(entry & 0x0FFFFFFFu);
	const int seg1 = (int)(entry >> 28);  // 0: the whole tile
	float4(*rec)[64] = s_rec[wave];
	uint32_t* recb = s_bands[wave];

	const int tx = tile % gx, ty = tile / gx;
	const int px = tx * GSR_TILE_X + (lane & 15);
	const int py0 = ty * GSR_TILE_Y + (lane >> 4);
	const v2f pfx2 = {(float)px, (float)px};
	const float x0f = (float)(tx * GSR_TILE_X), y0f = (float)(ty * GSR_TILE_Y);

	const uint2 range = ranges[tile];
	const int n = (int)min(range.y - range.x, tile_max_contrib[tile]);  // the tail was never blended
	int seg_a = 0, top = n;   // positions [seg_a, top) of the walk are this wave's
	if (seg1) {               // (binning.hip gsr_tile_segments: the same cut; its coarseness sits behind the list's last entry)
		const int coarse = (int)__builtin_amdgcn_readfirstlane(tile_order[nslots]);
		const int nblk = (n + GSR_CKPT_STRIDE - 1) / GSR_CKPT_STRIDE, m = (nblk + GSR_CKPT_MAX_SEGMENTS - 1) / GSR_CKPT_MAX_SEGMENTS * coarse;
		seg_a = (seg1 - 1) * m * GSR_CKPT_STRIDE;
		top = min(n, seg1 * m * GSR_CKPT_STRIDE);
	}
	const int nw = top - seg_a;
	const uint32_t* plist = point_list + range.x;
	const uint8_t* pmask = band_masks + range.x;
	const size_t plane = (size_t)H * W;
	const float bg0 = bg[0], bg1 = bg[1], bg2 = bg[2];
	const float ddelx_dx = 0.5f * W, ddely_dy = 0.5f * H;

	// Per-pixel state as two float2 "pixel pairs" per lane: pair p holds pixel slots k = 2p, 2p+1
	// (rows py0 + 8p and py0 + 8p + 4).  All add/mul/fma on pairs compile to v_pk_*_f32 -- two pixels
	// per VALU issue slot, which is what bounds this kernel (PMC: VALU active ~100 % of the time).
	// 36 registers of state for 4 pixels, so that 4 waves fit per SIMD.
	v2f T[2], tfb[2];                 // running T; -T_final * (bg . dL/dpix)
	v2f ac0[2], ac1[2], ac2[2];       // accum_rec as the NEXT hit will see it
	v2f dp0[2], dp1[2], dp2[2];
	v2f dpD[2], acD[2];               // AUX only: dL/dD, the depth channel's accum_rec
	int last_contributor[GSR_PIX_PER_LANE];
	v2f pfy[2];
#pragma unroll
	for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
		const int py = py0 + 4 * k;
		const bool inside = px < W && py < H;
		const uint32_t pix_id = inside ? (uint32_t)(W * py + px) : 0u;
		const float Tf = inside ? final_Ts[pix_id] : 0.f;
		const float d0 = inside ? dL_dpixels[pix_id] : 0.f;
		const float d1 = inside ? dL_dpixels[plane + pix_id] : 0.f;
		const float d2 = inside ? dL_dpixels[2 * plane + pix_id] : 0.f;
		last_contributor[k] = inside ? (int)n_contrib[pix_id] : 0;
		T[k >> 1][k & 1] = Tf;
		dp0[k >> 1][k & 1] = d0; dp1[k >> 1][k & 1] = d1; dp2[k >> 1][k & 1] = d2;
		if (AUX) {
			const float dD = (inside && aux.dL_ddepth) ? aux.dL_ddepth[pix_id] : 0.f;
			const float dA = (inside && aux.dL_dalpha) ? aux.dL_dalpha[pix_id] : 0.f;
			dpD[k >> 1][k & 1] = dD;
			tfb[k >> 1][k & 1] = -Tf * ((bg0 * d0 + bg1 * d1 + bg2 * d2) - dA);
		} else {
			tfb[k >> 1][k & 1] = -Tf * (bg0 * d0 + bg1 * d1 + bg2 * d2);
		}
		pfy[k >> 1][k & 1] = (float)py;
	}
#pragma unroll
	for (int p = 0; p < 2; p++) {
		ac0[p] = ac1[p] = ac2[p] = v2f{0.f, 0.f};
		if (AUX) acD[p] = v2f{0.f, 0.f};
	}
	if (top < n) {
		// The walk starts in the middle of the list.  The forward stored every pixel's (T, C) before the instance at position
		// `top`; what lies behind it blended to C_final - C, seen through T: the running T is the checkpoint's, and accum_rec --
		// the colour accumulated behind the current instance, backward.cu:553 -- is (C_final - C) / T.  A pixel whose last
		// contributor lies in front of `top` (n_contrib <= top) has nothing behind the segment: it starts from its final state,
		// T_final and 0, like a whole-tile walk -- and its checkpoint is not read (a band wave of the forward that finished early
		// wrote none).
		const float4* ck = checkpoints + ((size_t)(range.x + (uint32_t)top) / GSR_CKPT_STRIDE) * 256 + lane;
#pragma unroll
		for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
			const int py = py0 + 4 * k;
			const bool inside = px < W && py < H;
			const uint32_t pix_id = inside ? (uint32_t)(W * py + px) : 0u;
			if (inside && last_contributor[k] > top) {
				const float4 c = ck[64 * k];
				const float inv = 1.0f / c.x;   // T before an instance that still contributed: > 1e-4
				T[k >> 1][k & 1] = c.x;
				ac0[k >> 1][k & 1] = (final_C[pix_id] - c.y) * inv;
				ac1[k >> 1][k & 1] = (final_C[plane + pix_id] - c.z) * inv;
				ac2[k >> 1][k & 1] = (final_C[2 * plane + pix_id] - c.w) * inv;
				if (AUX) acD[k >> 1][k & 1] = (aux.final_D[pix_id] - aux.ckpt_depth[((size_t)(range.x + (uint32_t)top) / GSR_CKPT_STRIDE) * 256 + lane + 64 * k]) * inv;
			}
		}
	}
	// wave-uniform: the largest n_contrib among the 64 pixels of each band; instances at or beyond it
	// were blended into none of them, so the staging lanes clear the band's bit and nothing of it is evaluated
	int band_last[GSR_PIX_PER_LANE];
#pragma unroll
	for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
		int m = last_contributor[k];
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, 64));
		band_last[k] = __builtin_amdgcn_readfirstlane(m);
	}

	// back to front: batch position q = base + lane maps to range position top - 1 - q (top = n for a whole tile, the end of the segment otherwise)
	float4 ra = make_float4(0, 0, 0, 0), rb = ra, rc = ra;   // (rc.w: the depth value v in the AUX variant)
	uint32_t sbase = 0u;  // first gradient slot of the staged Gaussian (dense per-Gaussian array, cache resident)
	// the band mask of a position of the walk as the forward left it: 0 outside the walk, 0xF where the array is not consulted
	// (RECOMPUTE keeps no masks: its tests are the positions' own, and the parent form of this loop is what it compiles to)
	auto mask_at = [&](int q) -> uint32_t {
		if (RECOMPUTE || q >= nw) return 0u;
		return cull ? (uint32_t)pmask[top - 1 - q] : 0xFu;
	};
	uint32_t m_cur = mask_at(lane);   // of the batch whose records are in ra, rb, rc; m_next: of the batch whose ids are in id_next
	if (RECOMPUTE ? lane < nw : m_cur != 0u) {
		const uint32_t id = plist[top - 1 - lane];
		const float4* p = reinterpret_cast<const float4*>(splat + id);
		ra = p[0]; rb = p[1]; rc = p[2];
		sbase = slot_base[id];
	}
	uint32_t id_next = (64 + lane < nw) ? plist[top - 1 - (64 + lane)] : 0u;
	uint32_t m_next = mask_at(64 + lane);
	const int out_index = lane >> 3;                  // 8-lane group c ends up holding the wave total of v[c]
	float* const red_w = s_red[wave] + lane * 9;                       // this lane's row
	// column lane / 8, rows (lane % 8) + 8 k.  (Two of the eight 8-lane groups share seven banks in each of these reads: 2 conflict
	// cycles per read, SQ_LDS_BANK_CONFLICT = 25 M per launch at C3.  Rows 8 (lane % 8) + k are conflict-free and were measured:
	// 0.4665 -> 0.464 ms, and the other summation order put one needle-splat fuzz case 2 % over its end-to-end bar on
	// dL/drotations (blend sums unchanged at 1e-6): not kept.)
	const float* const red_r = s_red[wave] + (lane & 7) * 9 + (lane >> 3);
	constexpr int red_step = 72;
	const float out_scale = (out_index >= 2 && out_index <= 4) ? -0.5f : 1.0f;
	const float k01 = out_index == 0 ? -ddelx_dx : -ddely_dy;   // backward.cu:574-575: dL/dmean2D is scaled by 0.5 W / 0.5 H
	// The flush's lanes: lane = 32 h + 8 i + g.  h = 0: value g of pending instance i; h = 1: 8-lane group g of the same instance's
	// v[8].  Each reads eight consecutive words of s_pend: the column sums (i, g, r = 0..7), or v[8] of lanes 8 g .. 8 g + 7.
	const int f_inst = (lane >> 3) & 3, f_val = lane & 7;
	float* const pend_w = s_pend[wave] + lane;
	const float* const pend_r = s_pend[wave] + f_inst * 128 + (lane >> 5) * 64 + f_val * 8;
	const float f_scale = (f_val >= 2 && f_val <= 4) ? -0.5f : 1.0f;
	const float f_k01 = f_val == 0 ? -ddelx_dx : -ddely_dy;
	const bool f_word = lane < 32 || f_val == 0;   // stores a value word (lanes 0-31) or the ninth word (first lane of each upper group)
	int npend = 0;          // wave-uniform: reduced instances waiting in s_pend
	uint32_t pend_j = 0u;   // wave-uniform: their batch indices j, eight bits each (unused bytes 0, so every lane reads inside rec)

	for (int base = 0; base < nw; base += 64) {
		uint32_t reach = m_cur;   // (0 beyond the walk)
		if constexpr (RECOMPUTE) reach = (base + lane < nw) ? (cull ? gsr_tile_band_mask(ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, x0f, y0f) : 0xFu) : 0u;
		// The bands that still have an instance to come: at or beyond a band's largest n_contrib this one was blended into none of
		// its pixels (c0 / c1 below false in all lanes).  Decided here, 64 instances per instruction, so that the walk below reads a
		// pair's mode out of two bits: a scalar chain of compares and selects in front of each pair's branch cost the step 1.5 %.
		const int position = top - 1 - (base + lane);   // in the full range
		uint32_t live = 0u;
#pragma unroll
		for (int k = 0; k < GSR_PIX_PER_LANE; k++) live |= position < band_last[k] ? 1u << k : 0u;
		// GSR_DEBUG_NO_CULL (and the A/B build without this): a pair lives while either of its bands does, and is evaluated whole
		if (!(cull && GSR_BWD_BAND_LAST)) live = ((live & 3u) ? 3u : 0u) | ((live & 12u) ? 12u : 0u);
		const uint32_t bands = reach & live;
		const bool keep = cull ? bands != 0u : reach != 0u;   // (without the cull every instance is staged)
		const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
		const int cnt = __popcll(mask);
		GSR_TILE_STAT(st_staged += (unsigned)cnt;)
		if (keep) {
			const int pos = gsr_mbcnt(mask);
			const uint32_t rmin = __float_as_uint(rb.z), rwh = __float_as_uint(rb.w);
			const uint32_t slot = sbase + ((uint32_t)ty - (rmin >> 16)) * (rwh & 0xffffu) + ((uint32_t)tx - (rmin & 0xffffu));
			rec[0][pos] = make_float4(ra.x, ra.x, ra.y, ra.y);  // mean x, y
			// conic a and c pre-multiplied by -0.5: a power of two commutes with every rounding of `power`, so its bits are the
			// forward's (gsr_pair_power_halved) with one packed multiply less per pair; the epilogue undoes it inside an FMA
			rec[1][pos] = make_float4(-0.5f * ra.z, -0.5f * ra.z, ra.w, ra.w);  // -0.5 conic a, conic b
			rec[2][pos] = make_float4(-0.5f * rb.x, -0.5f * rb.x, rb.y, rb.y);  // -0.5 conic c, opacity
			rec[3][pos] = make_float4(rc.x, rc.x, rc.y, rc.y);  // r, g
			rec[4][pos] = make_float4(rc.z, rc.z, __int_as_float(position), __uint_as_float(slot));  // b, position in the full range, slot
			if (AUX) rec[5][pos] = make_float4(rc.w, rc.w, 0.f, 0.f);   // depth value v
			recb[pos] = bands | (reach << 4);   // (bits 4..7: the band mask alone, for the diagnostic counters)
		}
		if (RECOMPUTE ? base + 64 + lane < nw : m_next != 0u) {   // survivors of the forward's test only: a lane that skips the gather keeps a stale record and is not staged
			const float4* p = reinterpret_cast<const float4*>(splat + id_next);
			ra = p[0]; rb = p[1]; rc = p[2];
			sbase = slot_base[id_next];
		}
		m_cur = m_next;
		id_next = (base + 128 + lane < nw) ? plist[top - 1 - (base + 128 + lane)] : 0u;
		m_next = mask_at(base + 128 + lane);
		__builtin_amdgcn_wave_barrier();

#pragma clang loop unroll(disable)
		for (int j = 0; j < cnt; j++) {
			const float4 R0 = rec[0][j], R1 = rec[1][j], R2 = rec[2][j], R3 = rec[3][j], R4 = rec[4][j];
			const int contributor = __builtin_amdgcn_readfirstlane(__float_as_int(R4.z));  // backward.cu:511-515; wave-uniform
			const uint32_t bands = __builtin_amdgcn_readfirstlane(recb[j]);                 // wave-uniform
			const v2f X = {R0.x, R0.y}, Y = {R0.z, R0.w}, CA = {R1.x, R1.y}, CB = {R1.z, R1.w}, CC = {R2.x, R2.y}, OP = {R2.z, R2.w};
			const v2f C0 = {R3.x, R3.y}, C1 = {R3.z, R3.w}, C2 = {R4.x, R4.y};
			v2f V = {0.f, 0.f};
			if (AUX) { const float4 R5 = rec[5][j]; V = v2f{R5.x, R5.y}; }
			const v2f dx = X - pfx2;
			const v2f ax2 = (CA * dx) * dx, bdx = CB * dx;  // this file is compiled with -ffp-contract=off
			// ABS: a dx + b dy = -2 ((-0.5 a) dx + (-0.5 b) dy): with b halved like a and c, a per-pixel term is one product and one
			// FMA on f dx, f dy; the factor 2 (exact) joins 0.5 W / 0.5 H at the store
			v2f CBh = {0.f, 0.f};
			// Two scalar partials, not the two more v2f partials the feature was first specified with: |.| is a source modifier of the
			// scalar add but not of the packed one, so a v2f partial would pay a separate pair of ANDs per term, and two v2f are
			// four registers where this instantiation has none to spare.  The order of summation is as fixed as for acc[]: a pair's
			// two moduli are added to each other first, then to the lane's sum over its pixels.
			float absx = 0.f, absy = 0.f;
			if constexpr (ABS) CBh = -0.5f * CB;
			// per-lane partial sums over its pixels (one float2 = two pixels, added at the end).  The
			// geometric terms are raw moments of f = G * dL/dG = o g with g = G dL/dalpha (sum f dx, f dy, f dx^2, f dx dy,
			// f dy^2).  Two of f's factors do not vary over a lane's sum: the opacity o is one value per instance, and dx is one
			// value per lane (its four pixels share their column).  So a lane accumulates only sum g (acc[5], the dL/dopacity
			// word as it always was), sum g dy (acc[1]) and sum g dy^2 (acc[4]); dx and dx^2 meet the lane's sums once per
			// reduced instance, and so does the opacity (the reduction below says why not later); the conic and the
			// 0.5*W / 0.5*H / -0.5 factors of backward.cu:574-594 meet the wave's totals.  Six accumulators of the nine words are left:
			// acc[i] is the lane's share of word i for i = 1, 4 .. 8; words 0, 2, 3 have none.
			v2f acc[GSR_BWD_NV + 1];   // [9]: dL/dv (AUX)
#pragma unroll
			for (int i = 0; i < GSR_BWD_NV + 1; i++)
				if (i != 0 && i != 2 && i != 3) acc[i] = v2f{-0.f, -0.f};  // x + (-0) is x for every x: the first pair's sums need no add
			unsigned long long any = 0ull;  // lanes with a hit, kept as a scalar mask: the loop's branches test masks, not ballots of bools
			// One pair in mode M (its reachable bands: 3 both, 1 the .x band, 2 the .y band): the same operations in the same order
			// on a v2f or on one half of every register pair.  A band left out could not have hit: its alpha would be forced to 0,
			// its state update the identity bit for bit, and its additions exact zeros.
			auto pair = [&](auto pc, auto mc) {
				constexpr int p = decltype(pc)::value, M = decltype(mc)::value;
				typedef gsr_half<M> Hf;
				typedef typename Hf::type V_t;
				// power = -0.5f * (a*dx*dx + c*dy*dy) - b*dx*dy in the reference's operation order (CA, CC carry the -0.5)
				const V_t dy = Hf::get(Y) - Hf::get(pfy[p]);
				const V_t power = (Hf::get(ax2) + (Hf::get(CC) * dy) * dy) - Hf::get(bdx) * dy;
				// __expf(x) = v_exp_f32(x * log2(e)) (the forward's form, same constant, same IEEE product): the two products as one
				// packed multiply
				const V_t pl = power * 1.44269504088896340736f;
				const V_t G = gsr_exp2(pl);
				const V_t og = Hf::get(OP) * G;
				const V_t araw = gsr_min99(og);
				// each ballot of ONE comparison is that comparison's own lane mask (no instruction); a ballot of the combined
				// bool costs a v_cndmask + v_cmp round trip through a VGPR
				bool hit0 = false, hit1 = false;
				unsigned long long hits = 0ull;
				if constexpr ((M & 1) != 0) {
					const bool c0 = contributor < last_contributor[2 * p], p0 = !(gsr_lo(power) > 0.0f), a0 = !(gsr_lo(araw) < 1.0f / 255.0f);
					hit0 = c0 && p0 && a0;
					hits = __builtin_amdgcn_ballot_w64(c0) & __builtin_amdgcn_ballot_w64(p0) & __builtin_amdgcn_ballot_w64(a0);
				}
				if constexpr ((M & 2) != 0) {
					const bool c1 = contributor < last_contributor[2 * p + 1], p1 = !(gsr_hi(power) > 0.0f), a1 = !(gsr_hi(araw) < 1.0f / 255.0f);
					hit1 = c1 && p1 && a1;
					hits |= __builtin_amdgcn_ballot_w64(c1) & __builtin_amdgcn_ballot_w64(p1) & __builtin_amdgcn_ballot_w64(a1);
				}
				GSR_TILE_STAT(st_pairs++;)
				if (hits == 0ull) return;  // wave-uniform
				GSR_TILE_STAT(st_pairs_hit++; st_lanes_hit += (unsigned)__popcll(hits);)
				any |= hits;  // (lanes without a hit add exact zeros below)
				// A pixel that did not hit runs the same update with alpha = 0, which is the identity on its state
				// bit for bit (1 - 0 = 1, rcp(1) = 1, T * 1 = T, 0 * c + 1 * acc = acc): no per-state selects
				const V_t alpha = Hf::select(hit0, hit1, araw);
				const V_t oma = 1.f - alpha;
				const V_t inv1ma = gsr_rcp(oma);  // 1 ulp; IEEE division changed no parity figure
				const V_t Tn = Hf::get(T[p]) * inv1ma;
				// accum_rec and (c - accum_rec) cancel heavily when neighbouring colours are close: reference
				// operation order, no contraction (backward.cu:553-559)
				// dL/dalpha = sum_c (colour_c - accum_rec_c) * dL/dpix_c (backward.cu:553-559), as an FMA chain on the three
				// differences.  The differences cancel heavily when neighbouring colours are close, so they are formed first and
				// exactly as the reference forms them; what follows only accumulates.
				const V_t d0 = Hf::get(C0) - Hf::get(ac0[p]), d1 = Hf::get(C1) - Hf::get(ac1[p]), d2 = Hf::get(C2) - Hf::get(ac2[p]);
				V_t dL_dalpha = gsr_fma(d2, Hf::get(dp2[p]), gsr_fma(d1, Hf::get(dp1[p]), d0 * Hf::get(dp0[p])));
				V_t dV = Hf::get(V);
				if (AUX) {   // the depth channel: the same term and update as a colour channel
					dV = Hf::get(V) - Hf::get(acD[p]);
					dL_dalpha = gsr_fma(dV, Hf::get(dpD[p]), dL_dalpha);
				}
				// accum_rec' = last_alpha * last_color + (1 - last_alpha) * accum_rec (backward.cu:553; the reference applies it
				// lazily at the NEXT hit, from the same operands), written as accum_rec + alpha * (colour - accum_rec) on the
				// difference above: one FMA per channel instead of two products and a sum, and the smaller rounding error of the
				// two forms.  (Measured: 0.577 -> 0.534 ms for the kernel, all parity bars kept -- the blend sums stay at
				// 4e-7 ... 1.4e-6 of the CPU oracle's double-precision sums on C2 / C3.  Two further shortcuts were measured and
				// rejected: f = (o G) dL/dalpha instead of (o dL/dalpha) G saves nothing and moves the needle-splat stress case to
				// 1.03e-5.)
				const V_t n0 = gsr_fma(alpha, d0, Hf::get(ac0[p]));
				const V_t n1 = gsr_fma(alpha, d1, Hf::get(ac1[p]));
				const V_t n2 = gsr_fma(alpha, d2, Hf::get(ac2[p]));
				dL_dalpha = gsr_fma(dL_dalpha, Tn, Hf::get(tfb[p]) * inv1ma);
				// zero the partials of the pixel that did not hit (dL_dalpha of such a pixel is not zero by itself)
				const V_t dla = Hf::select(hit0, hit1, dL_dalpha);
				const V_t dch = alpha * Tn;             // dchannel_dcolor; 0 without a hit
				Hf::set(T[p], Tn);
				Hf::set(ac0[p], n0);
				Hf::set(ac1[p], n1);
				Hf::set(ac2[p], n2);
				if (AUX) {
					Hf::set(acD[p], gsr_fma(alpha, dV, Hf::get(acD[p])));
					Hf::set(acc[9], gsr_fma(dch, Hf::get(dpD[p]), Hf::get(acc[9])));   // dL/dv = alpha T dL/dD
				}
				Hf::set(acc[6], gsr_fma(dch, Hf::get(dp0[p]), Hf::get(acc[6])));
				Hf::set(acc[7], gsr_fma(dch, Hf::get(dp1[p]), Hf::get(acc[7])));
				Hf::set(acc[8], gsr_fma(dch, Hf::get(dp2[p]), Hf::get(acc[8])));
				Hf::set(acc[5], gsr_fma(G, dla, Hf::get(acc[5])));  // dL/dopacity = sum g, g = G dL/dalpha: also the x moments' sum
				const V_t g = G * dla;
				const V_t gdy = g * dy;
				Hf::set(acc[1], Hf::get(acc[1]) + gdy);
				Hf::set(acc[4], gsr_fma(gdy, dy, Hf::get(acc[4])));
				if constexpr (ABS) {   // a pixel without a hit has f = 0: it adds exact zeros here as above
					// the per-pixel moduli alone still need f = dL/dG * G and its two products; the nine words come from the sums above
					const V_t dxh = Hf::get(dx);
					const V_t f = (Hf::get(OP) * dla) * G;
					const V_t fdx = f * dxh, fdy = f * dy;
					const V_t tx = gsr_fma(Hf::get(CA), fdx, Hf::get(CBh) * fdy), ty = gsr_fma(Hf::get(CC), fdy, Hf::get(CBh) * fdx);
					absx += gsr_abs_sum(tx);
					absy += gsr_abs_sum(ty);
				}
			};
			auto pair_of = [&](auto pc) {
				constexpr int p = decltype(pc)::value;
				const uint32_t m = (bands >> (2 * p)) & 3u;   // wave-uniform: the pair's bands that can be reached and have an instance left
				if constexpr (ONE_BAND) {
					GSR_TILE_STAT(if (m == 1u || m == 2u) { if (((bands >> (4 + 2 * p)) & 3u) == m) st_one_mask++; else st_one_last++; })
					// Three if-then triangles in a row, not an if-else chain: the backend structurizes every diamond, uniform or not,
					// into guarded blocks whose state can no longer be updated in place (measured in the ISA: 131 v_mov in this loop
					// and 27 registers spilled, against 23 and none).  The two copies of m are opaque so that the tests stay apart.
					uint32_t m1 = m, m2 = m;
					asm volatile("" : "+s"(m1));
					asm volatile("" : "+s"(m2));
					if (m == 3u) pair(pc, std::integral_constant<int, 3>());
					if (m1 == 1u) pair(pc, std::integral_constant<int, 1>());
					if (m2 == 2u) pair(pc, std::integral_constant<int, 2>());
				} else {
					if (m != 0u) pair(pc, std::integral_constant<int, 3>());
				}
			};
			pair_of(std::integral_constant<int, 0>());
			pair_of(std::integral_constant<int, 1>());
			if (any) {  // wave-uniform
				GSR_TILE_STAT(st_reductions++;)
				float v[GSR_BWD_NV];
#pragma unroll
				for (int i = 0; i < GSR_BWD_NV; i++)
					if (i != 0 && i != 2 && i != 3) v[i] = gsr_add_halves(acc[i]);
				// the lane's dx on its sums: sum g dx = dx sum g, sum g dx^2 = dx (dx sum g), sum g dx dy = dx sum g dy
				v[0] = dx.x * v[5];
				v[2] = dx.x * v[0];
				v[3] = dx.x * v[1];
				// ... and the instance's opacity on the five geometric words: sums of g become sums of f = o g.  Per lane, before the
				// transposition, not once on the wave's totals (two instructions per reduced instance cheaper, measured first): a
				// rounding of a whole word is one error of 2^-24 of it that the other words do not share, and dL/dscales and
				// dL/drotations of a thin splat are differences of the three conic words that cancel a thousandfold -- one heavy-tile
				// fuzz scene then left dL/drotations 43 % over its end-to-end bar.  64 lanes' roundings average out, as the per-pixel
				// roundings of f did.
#pragma unroll
				for (int i = 0; i < 5; i++) v[i] *= OP.x;
				// the wave reduction of the first eight values through LDS: 64 x 8 partials in, transposed out -- the cross-lane work
				// is LDS traffic (its own issue port) plus 7 adds and the 3 DPP steps inside an 8-lane group, instead of 6 lane swaps,
				// 6 adds, 2 selects and 4 DPP steps on the vector ALU, which is what bounds this kernel.  A wave's LDS operations
				// execute in program order: the loads below see all 64 rows, and the next instance's stores come after them.
#pragma unroll
				for (int i = 0; i < 8; i++) red_w[i] = v[i];
				float col[8];
#pragma unroll
				for (int k = 0; k < 8; k++) col[k] = red_r[red_step * k];
				if constexpr (AUX || ABS) {
					// the ninth value's DPP chain runs while the LDS round trip is under way
					__builtin_amdgcn_sched_barrier(0);
					const float t9 = gsr_wave_sum_to_lane63(v[8]);  // lane 63 holds the total of v[8]
					float t10 = 0.f, tax = 0.f, tay = 0.f;
					if constexpr (AUX) t10 = gsr_wave_sum_to_lane63(gsr_add_halves(acc[9]));   // ... and of dL/dv
					if constexpr (ABS) {   // ... and of the two sums of moduli
						tax = gsr_wave_sum_to_lane63(absx);
						tay = gsr_wave_sum_to_lane63(absy);
					}
					__builtin_amdgcn_sched_barrier(0);
					const float tcol = ((col[0] + col[1]) + (col[2] + col[3])) + ((col[4] + col[5]) + (col[6] + col[7]));
					const float t8 = gsr_sum8(tcol);                // group c holds the total of v[c]
					// dL/dmean2D: group 0 (sum f dx = sx) needs sy, group 1 (sy) needs sx -- the partner half row, one DPP move; the
					// same products and the same FMA as the scalar form below (a sx + b sy with a = -2 (-0.5 a)), so the same bits
					const float other = gsr_dpp_mov<0x128, 0xF, 0xF, true>(t8);  // row_ror:8
					const float r01 = k01 * __builtin_fmaf(-2.0f, (out_index == 0 ? CA.x : CC.x) * t8, CB.x * other);
					const uint32_t slot = __builtin_amdgcn_readfirstlane(__float_as_uint(R4.w));
					float* out = reinterpret_cast<float*>(slots + slot);
					const float r = out_index < 2 ? r01 : out_scale * t8;   // dL/dconic .x .y .w (x -0.5); opacity and colour as they are
					if ((lane & 7) == 0) out[out_index] = r;
					if (lane == 63) {
						if constexpr (ABS) {   // words 8..11 as one 16-byte store (pad0 is 0 without AUX)
							reinterpret_cast<float4*>(out)[2] = make_float4(t9, t10, (2.0f * ddelx_dx) * tax, (2.0f * ddely_dy) * tay);
						} else {
							out[8] = t9;
							out[9] = t10;
						}
						slot_valid[slot] = 1;
					}
				} else {
					// Everything after the column sums waits for the flush: this lane's column sum and its v[8] go to the
					// instance's place in s_pend, its batch index j to pend_j.  The 7 adds below are all the per-instance work left.
					const float tcol = ((col[0] + col[1]) + (col[2] + col[3])) + ((col[4] + col[5]) + (col[6] + col[7]));
					pend_w[npend * 128] = tcol;
					pend_w[npend * 128 + 64] = v[8];
					pend_j |= (uint32_t)j << (8 * npend);
					npend++;
				}
			}
			if (!(AUX || ABS) && (npend == GSR_BWD_FLUSH || (npend != 0 && j == cnt - 1))) {  // wave-uniform; rec is restaged only after the batch
				// gsr_flush: finish up to four reduced instances in one instruction stream over the 64 lanes.  A wave's LDS
				// operations execute in program order, so the reads below see every s_pend store above, and the next instance's
				// stores come after them; the wave barriers only keep the compiler from moving LDS accesses across.
				__builtin_amdgcn_wave_barrier();
				const float4 q0 = *reinterpret_cast<const float4*>(pend_r), q1 = *reinterpret_cast<const float4*>(pend_r + 4);
				// the instance's epilogue scalars, still staged in rec: -0.5 conic a and b (rec[1]), -0.5 conic c (rec[2]), slot (rec[4])
				const uint32_t jf = (pend_j >> (8 * f_inst)) & 0xFFu;
				const float* const rj = reinterpret_cast<const float*>(&rec[0][jf]);
				const float ca = rj[4 * 64], cb = rj[4 * 64 + 2], cc = rj[8 * 64];
				const uint32_t slot = __float_as_uint(rj[16 * 64 + 3]);
				// one LDS round trip for all six reads: left alone, the compiler sinks the scalars' reads into the store branch below
				// and waits for them a second time
				asm volatile("" ::"v"(q0.x), "v"(q1.x), "v"(ca), "v"(cb), "v"(cc), "v"(slot));
				// lanes 0-31: value g's eight column sums, r = 0..7, added as gsr_sum8 adds the lanes (g, 0..7) of the per-instance
				// form -- quad_perm [1,0,3,2] pairs (0,1) ... (6,7), quad_perm [2,3,0,1] pairs the pairs, row_half_mirror the
				// quads: ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)), each add's operand order aside, which fp32 addition does not see.
				// lanes 32-63: the same tree over v[8] of lanes 8 g .. 8 g + 7 is S_g, the value gsr_wave_sum_to_lane63 has in
				// every lane of group g after its first three steps.  Its row_mirror step makes R_k = S_2k + S_2k+1, row_bcast:15
				// leaves R3 + R2 in lane 63, row_bcast:31 adds R1 + R0 (lane 31): (R0+R1)+(R2+R3).  gsr_sum8 over S_0..S_7 is
				// (S0+S1)+(S2+S3) = R0+R1 in the first quad and R2+R3 in the second, then their sum: the same total, bit for bit.
				const float t = ((q0.x + q0.y) + (q0.z + q0.w)) + ((q1.x + q1.y) + (q1.z + q1.w));
				const float t9 = gsr_sum8(t);   // lanes 32-63: the instance's total of v[8]
				// dL/dmean2D: value 0 (sum f dx = sx) needs sy, value 1 needs sx -- the neighbouring lane, one DPP move; the same
				// products and the same FMA as the per-instance form (a sx + b sy with a = -2 (-0.5 a))
				const float other = gsr_dpp_mov<0xB1, 0xF, 0xF, true>(t);  // quad_perm [1,0,3,2]
				const float r01 = f_k01 * __builtin_fmaf(-2.0f, (f_val == 0 ? ca : cc) * t, cb * other);
				const float r = f_val < 2 ? r01 : f_scale * t;   // dL/dconic .x .y .w (x -0.5); opacity and colour as they are
				if (f_inst < npend) {
					if (f_word) reinterpret_cast<float*>(slots + slot)[lane < 32 ? f_val : 8] = lane < 32 ? r : t9;
					if (lane >= 32 && f_val == 0) slot_valid[slot] = 1;
				}
				npend = 0;
				pend_j = 0u;
				__builtin_amdgcn_wave_barrier();
			}
		}
		__builtin_amdgcn_wave_barrier();
	}
	GSR_TILE_CLOCK_STOP(gsr_backward_tile_clock, slot_id, lane, st_staged | (st_pairs << 20) | (st_pairs_hit << 42), st_reductions | (st_lanes_hit << 24), st_one_mask | (st_one_last << 32));   // one record per dispatch entry
}

#define GSR_BWD_KERNEL(name, RECOMPUTE)                                                                                                        \
	template <bool AUX, bool ABS>                                                                                                              \
	__global__ void __launch_bounds__(64 * GSR_WAVES_PER_WG) __attribute__((amdgpu_waves_per_eu((AUX && ABS) ? 3 : 4, 4))) name(                \
		int W, int H, int gx, int nslots, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,                           \
		const uint8_t* __restrict__ band_masks, const GsrSplat* __restrict__ splat, const float4* __restrict__ checkpoints,                    \
		const float* __restrict__ final_C, const uint32_t* __restrict__ slot_base, const float* __restrict__ bg,                               \
		const float* __restrict__ final_Ts, const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max_contrib,             \
		const uint32_t* __restrict__ tile_order, const float* __restrict__ dL_dpixels, GsrGradSlot* __restrict__ slots,                        \
		uint8_t* __restrict__ slot_valid, int cull, GsrAuxBlend aux)                                                                           \
	{                                                                                                                                          \
		gsr_render_backward_wave<AUX, ABS, RECOMPUTE>(W, H, gx, nslots, ranges, point_list, band_masks, splat, checkpoints, final_C, slot_base, bg, \
		                                              final_Ts, n_contrib, tile_max_contrib, tile_order, dL_dpixels, slots, slot_valid, cull, aux); \
	}
GSR_BWD_KERNEL(gsr_render_backward_wave_kernel, false)             // the band masks are the forward's
GSR_BWD_KERNEL(gsr_render_backward_recompute_kernel, true)         // GSR_DEBUG_RECOMPUTE_BANDS
#undef GSR_BWD_KERNEL

void gsr_launch_render_backward(const GsrFrame& f, const float* bg, const float* dL_dpix, hipEvent_t t_start, hipEvent_t t_stop,
                                const GsrAuxBlend* aux, bool absgrad)
{
	const GsrImage& img = f.img;
	const int W = f.W, H = f.H, gx = gsr_grid_x(W), gy = gsr_grid_y(H);
	const int ntiles = gx * gy;
	const int nslots = ntiles + (int)gsr_tile_order_max_segments(ntiles);   // whole tiles + the extra entries of heavy tiles' depth segments
	const int nwg = (nslots + GSR_WAVES_PER_WG - 1) / GSR_WAVES_PER_WG;
	// (one kernel for both modes of the maps: it reads v from the record; the blend has no anti-aliased form, so the third slot of
	// gsr_variant carries ABS here)
	// (... and the first, which no blend kernel has a use for, carries GSR_DEBUG_RECOMPUTE_BANDS)
	gsr_variant((f.debug & GSR_DEBUG_RECOMPUTE_BANDS) != 0, aux ? GSR_AUX_DEPTH : 0, absgrad, [&](auto RECOMPUTE, auto AUX, auto ABS) {
		auto kernel = gsr_render_backward_wave_kernel<AUX() != 0, ABS()>;
		if (RECOMPUTE()) kernel = gsr_render_backward_recompute_kernel<AUX() != 0, ABS()>;
		gsr_launch(kernel, dim3(nwg), dim3(64 * GSR_WAVES_PER_WG), 0, f.s, t_start, t_stop, W, H, gx, nslots,
		           img.ranges, f.bin.point_list, f.bin.band_masks, f.g.splat, f.bin.checkpoints, img.final_C, f.g.slot_base, bg, img.final_T, img.n_contrib,
		           img.tile_max_contrib, img.tile_order, dL_dpix, f.slots, f.slot_valid, f.cull ? 1 : 0, aux ? *aux : GsrAuxBlend{});
	});
}
