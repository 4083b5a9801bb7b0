// features.hip -- K per-Gaussian feature channels blended with the colour pass's own weights, and their gradients
// (include/gsr_features.h): F_k(p) = sum_i f_ik alpha_i T_i(p), no background term.  Three kernels, no atomics, no workgroup
// barrier, bitwise reproducible.  None of the default kernels is touched: the passes below read the state a forward of any variant
// left, the way contrib.hip does.
//
// Decomposition (render_common.h): one wave64 per 16x16 tile, four pixels per lane, 64 instances staged per batch into the wave's LDS
// slice behind gsr_tile_band_mask (`cull`).  The channels are processed in chunks of GSR_FEAT_CH = 4 -- 16 accumulators per lane --
// a ragged last chunk is padded with zero features and zero gradients inside the kernels.  A chunk is one wave's whole walk:
//   forward         grid (tiles, chunks): the chunks of one tile are independent waves of one launch;
//   backward tiles  into_slots = 0: grid (tiles, chunks) as the forward; into_slots = 1: one launch per chunk, in chunk order on the
//                   stream, because every chunk adds into the same six words of the gradient slot (see below) -- the order of these
//                   additions is the launch order, so the sum is reproducible.
//
// Forward tile pass: the forward's walk over again, as gsr_contrib_tiles_kernel walks it -- the list positions
// [0, min(range length, tile_max_contrib)), for a pixel only the positions in front of its n_contrib; `power`, alpha, the two
// thresholds and T's update are render_forward.hip's instruction sequence on the same records (gsr_pair_power_halved, __expf,
// fminf(0.99, .), __fmul_rn, __fsub_rn), so w = alpha T has the colour pass's bits and F_k = fma(f_ik, w, F_k), in list order, is
// what the colour kernel would have accumulated for a colour f_ik.  out[K][H][W] is written in full (zeros where nothing blends);
// nothing of the state is written.
//
// Backward tile pass: backward.cu:507-599 per pixel with the chunk's four channels in place of the three colours and a zero
// background: back to front from final_T and n_contrib, T_i = T_{i+1} / (1 - alpha_i) (v_rcp_f32, as render_backward.hip),
// accum_rec per channel, the straight-through 0.99 clamp, dL/dalpha_i = sum_k (f_ik - accum_rec_k) g_k T_i with g = dL/dF.
// Per (Gaussian, tile) instance with at least one hit the wave reduces
//   (a) the four sums over the pixels of alpha T g_k -- dL/df_ik of this tile -- into the instance's own 16-byte record of the
//       features scratch (chunk c, slot s: record c * R + s; slot numbering of the gradient slots, render_backward.hip), and sets the
//       slot's validity byte (one byte per slot behind the records; the chunks of a call hit the same instances, so they share it);
//   (b) SLOTS only: the raw moments sum f dx, f dy, f dx^2, f dx dy, f dy^2 of f = G dL/dG and sum G dL/dalpha, finished by the
//       epilogue algebra of render_backward.hip (a sx + b sy scaled by -0.5 W / -0.5 H, -0.5 on the conic moments) and ADDED into
//       words 0..5 of the GsrGradSlot the colour blend wrote for the same instance: a plain read-modify-write by lanes 0..5 of the
//       one wave that owns the tile in this launch.  Words 6..11 are not touched.  The hit set is the colour blend's (same records,
//       same n_contrib, same thresholds), so exactly the slots it validated are updated and the unchanged per-Gaussian backward
//       chains the total.
// Reduction: every reduced instance is finished on its own through LDS -- each lane stores its NV partials (4, or 10 with SLOTS) into
// NV rows of 64 words (row stride 80: the rows of one 8-lane read group sit 16 banks apart, contrib.hip), lane (v, q) = 4 v + q reads
// the 16 words of quarter q of row v with four ds_read_b128 and folds them, two lane exchanges join the quarters, and the totals
// are broadcast as scalars (v_readlane_b32) for the epilogue.  Per reduced instance: NV ds_write_b32, 4 ds_read_b128, 17 adds,
// 2 ds_bpermute_b32 -- the cross-lane work stays on the LDS pipe, as in contrib.hip and render_backward.hip; neither parking
// (contrib.hip's flush) nor the 64 x 9 transpose is used: with ten values the four-instance flush would not fit 64 lanes.
// Heavy tiles are walked whole by one wave (no depth segments): the launch's tail is the longest list of the view.
//
// Per-Gaussian fold: one lane per Gaussian adds its run of feature records [slot_base[g], + tiles_touched[g]) in index order, chunk
// by chunk, and writes all K elements of dL_dfeatures[g] (zeros without a hit: the caller's memory may be uninitialised).
//
// Registers (hipcc 7.x, gfx950, -O3 -ffp-contract=off; `make audit`, .audit/features.s):
//   gsr_features_forward_kernel             84 VGPRs, 5 waves per SIMD, no scratch
//   gsr_features_backward_kernel<false>     96 VGPRs, 5 waves per SIMD, no scratch
//   gsr_features_backward_kernel<true>     124 VGPRs, 4 waves per SIMD, no scratch
//   gsr_features_fold_kernel                16 VGPRs, 8 waves per SIMD, no scratch
// No kernel spills to scratch (ScratchSize 0, private_segment_fixed_size 0 for all four).
// LDS per wave: forward 3 328 bytes, backward 8 448 bytes (20 waves of the backward: 165 KB -- a CU's 160 KB hold 19, so the
// <false> instantiation is bound by LDS at 19 waves per CU just below its register limit; <true> runs its 16).
#include "render_common.h"

#define GSR_FEAT_CH 4
#define GSR_FEAT_ROW 80     // words between two rows of the reduction area (contrib.hip GSR_CONTRIB_ROW)
#define GSR_FEAT_ROWS 16    // rows allocated: lane 4 v + q reads row v, v = 0..15, whatever NV is

// the chunk's four features of Gaussian `id`, zeros beyond channel K - 1
__device__ __forceinline__ float4 gsr_feat_load(const float* __restrict__ features, uint32_t id, int K, int ch0)
{
	const float* f = features + (size_t)id * (size_t)K + ch0;
	float4 r;
	r.x = f[0];   // ch0 < K always
	r.y = ch0 + 1 < K ? f[1] : 0.f;
	r.z = ch0 + 2 < K ? f[2] : 0.f;
	r.w = ch0 + 3 < K ? f[3] : 0.f;
	return r;
}

__global__ void __launch_bounds__(64 * GSR_WAVES_PER_WG) gsr_features_forward_kernel(
	int W, int H, int gx, int ntiles, int K, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
	const GsrSplat* __restrict__ splat, const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max_contrib,
	const float* __restrict__ features, float* __restrict__ out, int cull)
{
	// the surviving instances of a batch: (x, y, -0.5 conic a, conic b), (-0.5 conic c, opacity, list position, -), the four features
	__shared__ float4 s_rec[GSR_WAVES_PER_WG][3][64];
	__shared__ uint32_t s_bands[GSR_WAVES_PER_WG][64];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int tile = blockIdx.x * GSR_WAVES_PER_WG + wave;
	if (tile >= ntiles) return;  // wave-uniform; no barriers below
	const int ch0 = GSR_FEAT_CH * (int)blockIdx.y;
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

	float T[GSR_PIX_PER_LANE], pfy[GSR_PIX_PER_LANE], F[GSR_PIX_PER_LANE][GSR_FEAT_CH];
	uint32_t last[GSR_PIX_PER_LANE];        // the pixel's n_contrib: it blended positions in front of this one only (0 outside the image)
	uint32_t band_last[GSR_PIX_PER_LANE];   // wave-uniform: the largest of them in band k
#pragma unroll
	for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
		const int py = py0 + 4 * k;
		const bool inside = px < W && py < H;
		const uint32_t pix_id = inside ? (uint32_t)(W * py + px) : 0u;
		pfy[k] = (float)py;
		T[k] = 1.0f;
#pragma unroll
		for (int c = 0; c < GSR_FEAT_CH; c++) F[k][c] = 0.f;
		last[k] = inside ? n_contrib[pix_id] : 0u;
		uint32_t m = last[k];
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
		band_last[k] = __builtin_amdgcn_readfirstlane(m);
	}

	// software pipeline: records one batch ahead, ids two batches ahead
	float4 ra = make_float4(0, 0, 0, 0), rb = ra, rf = ra;
	if (lane < n) {
		const uint32_t id = plist[lane];
		const float4* p = reinterpret_cast<const float4*>(splat + id);
		ra = p[0]; rb = p[1];
		rf = gsr_feat_load(features, id, K, ch0);
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
			rec[1][pos] = make_float4(-0.5f * rb.x, rb.y, __uint_as_float((uint32_t)(base + lane)), 0.f);
			rec[2][pos] = rf;
			recb[pos] = bands;
		}
		if (base + 64 + lane < n) {
			const float4* p = reinterpret_cast<const float4*>(splat + id_next);
			ra = p[0]; rb = p[1];
			rf = gsr_feat_load(features, id_next, K, ch0);
		}
		id_next = (base + 128 + lane < n) ? plist[base + 128 + lane] : 0u;
		__builtin_amdgcn_wave_barrier();

		for (int j = 0; j < cnt; j++) {
			const float4 A = rec[0][j];   // x, y, -0.5 conic a, conic b
			const float4 B = rec[1][j];   // -0.5 conic c, opacity, list position
			const float4 Fj = rec[2][j];
			const uint32_t position = __builtin_amdgcn_readfirstlane(__float_as_uint(B.z));   // wave-uniform
			const uint32_t jbands = __builtin_amdgcn_readfirstlane(recb[j]);                  // wave-uniform
			const float dx = A.x - pfx;
			const float ax2 = __fmul_rn(__fmul_rn(A.z, dx), dx), bdx = __fmul_rn(A.w, dx);
#pragma unroll
			for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
				if (!(jbands & (1u << k)) || position >= band_last[k]) continue;  // scalar branch: the band cannot be reached, or it had finished
				const float dy = A.y - pfy[k];
				const float power = gsr_pair_power_halved(ax2, bdx, B.x, dy);
				const float alpha = fminf(0.99f, B.y * __expf(power));
				const unsigned long long hitm = __builtin_amdgcn_ballot_w64(position < last[k]) & __builtin_amdgcn_ballot_w64(!(power > 0.0f)) &
				                                __builtin_amdgcn_ballot_w64(!(alpha < 1.0f / 255.0f));
				if (hitm == 0ull) continue;  // wave-uniform
				const bool hit = __builtin_amdgcn_inverse_ballot_w64(hitm);
				const float w = hit ? __fmul_rn(alpha, T[k]) : 0.0f;                  // the forward's alpha * T
				T[k] = hit ? __fmul_rn(T[k], __fsub_rn(1.0f, alpha)) : T[k];          // ... and its T (1 - alpha), rounded as there
				F[k][0] = __builtin_fmaf(Fj.x, w, F[k][0]);
				F[k][1] = __builtin_fmaf(Fj.y, w, F[k][1]);
				F[k][2] = __builtin_fmaf(Fj.z, w, F[k][2]);
				F[k][3] = __builtin_fmaf(Fj.w, w, F[k][3]);
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
#pragma unroll
			for (int c = 0; c < GSR_FEAT_CH; c++)
				if (ch0 + c < K) out[(size_t)(ch0 + c) * plane + pix_id] = F[k][c];
		}
	}
}

// SLOTS: also the six geometry quantities, added into words 0..5 of the instance's gradient slot (grid.y must be 1: one chunk per launch)
template <bool SLOTS>
__global__ void __launch_bounds__(64 * GSR_WAVES_PER_WG) gsr_features_backward_kernel(
	int W, int H, int gx, int ntiles, int K, int chunk0, uint32_t R, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
	const GsrSplat* __restrict__ splat, const uint32_t* __restrict__ slot_base, const float* __restrict__ final_Ts,
	const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max_contrib, const float* __restrict__ features,
	const float* __restrict__ dL_dout, float4* __restrict__ frec, uint8_t* __restrict__ fvalid, GsrGradSlot* slots, int cull)
{
	constexpr int NV = SLOTS ? GSR_FEAT_CH + 6 : GSR_FEAT_CH;
	// the surviving instances of a batch: (x, y, -0.5 conic a, conic b), (-0.5 conic c, opacity, list position, slot), the four features
	__shared__ float4 s_rec[GSR_WAVES_PER_WG][3][64];
	__shared__ uint32_t s_bands[GSR_WAVES_PER_WG][64];
	// reduction area: row v holds the 64 lanes' partial v of the instance being reduced
	__shared__ __attribute__((aligned(16))) float s_red[GSR_WAVES_PER_WG][GSR_FEAT_ROWS * GSR_FEAT_ROW];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int tile = blockIdx.x * GSR_WAVES_PER_WG + wave;
	if (tile >= ntiles) return;  // wave-uniform; no barriers below
	const int chunk = chunk0 + (int)blockIdx.y;
	const int ch0 = GSR_FEAT_CH * chunk;
	float4(*rec)[64] = s_rec[wave];
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
	float ar[GSR_PIX_PER_LANE][GSR_FEAT_CH];   // accum_rec as the NEXT hit will see it
	float g[GSR_PIX_PER_LANE][GSR_FEAT_CH];    // dL/dF of the pixel
	uint32_t last[GSR_PIX_PER_LANE], band_last[GSR_PIX_PER_LANE];
#pragma unroll
	for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
		const int py = py0 + 4 * k;
		const bool inside = px < W && py < H;
		const size_t pix_id = inside ? (size_t)W * py + px : 0;
		pfy[k] = (float)py;
		T[k] = inside ? final_Ts[pix_id] : 0.f;
		last[k] = inside ? n_contrib[pix_id] : 0u;
#pragma unroll
		for (int c = 0; c < GSR_FEAT_CH; c++) {
			ar[k][c] = 0.f;
			g[k][c] = (inside && ch0 + c < K) ? dL_dout[(size_t)(ch0 + c) * plane + pix_id] : 0.f;
		}
		uint32_t m = last[k];
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
		band_last[k] = __builtin_amdgcn_readfirstlane(m);
	}

	// back to front: batch position q = base + lane maps to list position n - 1 - q
	float4 ra = make_float4(0, 0, 0, 0), rb = ra, rf = ra;
	uint32_t sbase = 0u;
	if (lane < n) {
		const uint32_t id = plist[n - 1 - lane];
		const float4* p = reinterpret_cast<const float4*>(splat + id);
		ra = p[0]; rb = p[1];
		rf = gsr_feat_load(features, id, K, ch0);
		sbase = slot_base[id];
	}
	uint32_t id_next = (64 + lane < n) ? plist[n - 1 - (64 + lane)] : 0u;
	// the reduction's reader: lane 4 v + q folds the words 16 q .. 16 q + 15 of row v
	const float* const red_r = red + (lane >> 2) * GSR_FEAT_ROW + 16 * (lane & 3);

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
			rec[2][pos] = rf;
			recb[pos] = bands;
		}
		if (base + 64 + lane < n) {
			const float4* p = reinterpret_cast<const float4*>(splat + id_next);
			ra = p[0]; rb = p[1];
			rf = gsr_feat_load(features, id_next, K, ch0);
			sbase = slot_base[id_next];
		}
		id_next = (base + 128 + lane < n) ? plist[n - 1 - (base + 128 + lane)] : 0u;
		__builtin_amdgcn_wave_barrier();

		for (int j = 0; j < cnt; j++) {
			const float4 A = rec[0][j];   // x, y, -0.5 conic a, conic b
			const float4 B = rec[1][j];   // -0.5 conic c, opacity, list position, slot
			const float4 Fj = rec[2][j];
			const uint32_t position = __builtin_amdgcn_readfirstlane(__float_as_uint(B.z));   // backward.cu:511-515; wave-uniform
			const uint32_t jbands = __builtin_amdgcn_readfirstlane(recb[j]);                  // wave-uniform
			const float fj[GSR_FEAT_CH] = {Fj.x, Fj.y, Fj.z, Fj.w};
			const float dx = A.x - pfx;
			const float ax2 = __fmul_rn(__fmul_rn(A.z, dx), dx), bdx = __fmul_rn(A.w, dx);
			// per-lane partial sums over its four pixels: [0..3] alpha T g_k; SLOTS: [4..8] the raw moments of f = G dL/dG
			// (f dx, f dy, f dx^2, f dx dy, f dy^2), [9] G dL/dalpha
			float acc[NV];
#pragma unroll
			for (int i = 0; i < NV; i++) acc[i] = 0.f;
			unsigned long long any = 0ull;  // lanes with a hit
#pragma unroll
			for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
				if (!(jbands & (1u << k)) || position >= band_last[k]) continue;  // scalar branch: the band cannot be reached, or none of its pixels blended this far
				const float dy = A.y - pfy[k];
				const float power = gsr_pair_power_halved(ax2, bdx, B.x, dy);
				const float G = __expf(power);
				const float araw = fminf(0.99f, B.y * G);
				const unsigned long long hitm = __builtin_amdgcn_ballot_w64(position < last[k]) & __builtin_amdgcn_ballot_w64(!(power > 0.0f)) &
				                                __builtin_amdgcn_ballot_w64(!(araw < 1.0f / 255.0f));
				if (hitm == 0ull) continue;  // wave-uniform
				any |= hitm;
				const bool hit = __builtin_amdgcn_inverse_ballot_w64(hitm);
				// a pixel that did not hit runs the same update with alpha = 0: the identity on its state, bit for bit
				const float alpha = hit ? araw : 0.f;
				const float inv1ma = __builtin_amdgcn_rcpf(1.f - alpha);
				const float Tn = T[k] * inv1ma;   // T in front of this instance
				// dL/dalpha = sum_c (f_c - accum_rec_c) g_c T: the differences first, as the reference forms them, then an FMA chain
				float d[GSR_FEAT_CH];
#pragma unroll
				for (int c = 0; c < GSR_FEAT_CH; c++) d[c] = fj[c] - ar[k][c];
				float dla = d[0] * g[k][0];
#pragma unroll
				for (int c = 1; c < GSR_FEAT_CH; c++) dla = __builtin_fmaf(d[c], g[k][c], dla);
				// accum_rec' = alpha f + (1 - alpha) accum_rec, on the difference above (render_backward.hip)
#pragma unroll
				for (int c = 0; c < GSR_FEAT_CH; c++) ar[k][c] = __builtin_fmaf(alpha, d[c], ar[k][c]);
				dla = hit ? dla * Tn : 0.f;   // (zero background: no T_final term)
				const float dch = alpha * Tn;  // dF/df; 0 without a hit
				T[k] = Tn;
#pragma unroll
				for (int c = 0; c < GSR_FEAT_CH; c++) acc[c] = __builtin_fmaf(dch, g[k][c], acc[c]);
				if constexpr (SLOTS) {
					acc[9] = __builtin_fmaf(G, dla, acc[9]);    // dL/dopacity
					const float f = (B.y * dla) * G;             // dL/dG * G (straight through the 0.99 clamp)
					const float fdx = f * dx, fdy = f * dy;
					acc[4] += fdx;
					acc[5] += fdy;
					acc[6] = __builtin_fmaf(fdx, dx, acc[6]);
					acc[7] = __builtin_fmaf(fdx, dy, acc[7]);
					acc[8] = __builtin_fmaf(fdy, dy, acc[8]);
				}
			}
			if (any == 0ull) continue;   // wave-uniform: nothing is written for an instance without a hit
			// the wave reduction.  A wave's LDS operations execute in program order: the reads see all 64 lanes' stores, and the
			// next instance's stores come after them; the wave barriers keep the compiler from moving LDS accesses across.
#pragma unroll
			for (int i = 0; i < NV; i++) red[i * GSR_FEAT_ROW + lane] = acc[i];
			__builtin_amdgcn_wave_barrier();
			const float4 q0 = *reinterpret_cast<const float4*>(red_r), q1 = *reinterpret_cast<const float4*>(red_r + 4);
			const float4 q2 = *reinterpret_cast<const float4*>(red_r + 8), q3 = *reinterpret_cast<const float4*>(red_r + 12);
			__builtin_amdgcn_wave_barrier();
			float t = (((q0.x + q0.y) + (q0.z + q0.w)) + ((q1.x + q1.y) + (q1.z + q1.w))) + (((q2.x + q2.y) + (q2.z + q2.w)) + ((q3.x + q3.y) + (q3.z + q3.w)));
			t += __shfl_xor(t, 1, 64);
			t += __shfl_xor(t, 2, 64);   // lanes 4 v .. 4 v + 3 hold the wave's total of value v (rows >= NV: never used)
			float S[NV];   // wave-uniform
#pragma unroll
			for (int i = 0; i < NV; i++) S[i] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(t), 4 * i));
			const uint32_t slot = __builtin_amdgcn_readfirstlane(__float_as_uint(B.w));
			if (lane == 0) {
				frec[(size_t)chunk * R + slot] = make_float4(S[0], S[1], S[2], S[3]);
				fvalid[slot] = 1;
			}
			if constexpr (SLOTS) {
				// render_backward.hip's epilogue: dL/dmean2D = -0.5 W (a sx + b sy), -0.5 H (c sy + b sx), with a = -2 (-0.5 a)
				// inside the FMA; dL/dconic .x .y .w = -0.5 x the second moments; dL/dopacity as it is
				const float ca = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(A.z)));
				const float cb = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(A.w)));
				const float cc = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(B.x)));
				const float r0 = -ddelx_dx * __builtin_fmaf(-2.0f, ca * S[4], cb * S[5]);
				const float r1 = -ddely_dy * __builtin_fmaf(-2.0f, cc * S[5], cb * S[4]);
				const float r = lane == 0 ? r0 : lane == 1 ? r1 : lane == 2 ? -0.5f * S[6] : lane == 3 ? -0.5f * S[7] : lane == 4 ? -0.5f * S[8] : S[9];
				if (lane < 6) {
					float* w = reinterpret_cast<float*>(slots + slot) + lane;
					*w = *w + r;
				}
			}
		}
		__builtin_amdgcn_wave_barrier();
	}
}

// one lane per Gaussian: its records of every chunk in index order; all K outputs are written
__global__ void __launch_bounds__(256) gsr_features_fold_kernel(int P, int K, uint32_t R, const uint32_t* __restrict__ tiles_touched,
                                                                const uint32_t* __restrict__ slot_base, const float4* __restrict__ frec,
                                                                const uint8_t* __restrict__ fvalid, float* __restrict__ dL_dfeatures)
{
	const int gi = blockIdx.x * 256 + threadIdx.x;
	if (gi >= P) return;
	const uint32_t tiles = tiles_touched[gi];
	const uint32_t base = tiles ? slot_base[gi] : 0u;   // culled: slot_base was never written
	float* out = dL_dfeatures + (size_t)gi * (size_t)K;
	for (int ch0 = 0; ch0 < K; ch0 += GSR_FEAT_CH) {
		const float4* rc = frec + (size_t)(ch0 / GSR_FEAT_CH) * R;
		float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
		for (uint32_t k = 0; k < tiles; k++) {
			if (!fvalid[base + k]) continue;
			const float4 r = rc[base + k];
			s.x += r.x; s.y += r.y; s.z += r.z; s.w += r.w;
		}
		out[ch0] = s.x;
		if (ch0 + 1 < K) out[ch0 + 1] = s.y;
		if (ch0 + 2 < K) out[ch0 + 2] = s.z;
		if (ch0 + 3 < K) out[ch0 + 3] = s.w;
	}
}

int gsr_features_chunks(int K) { return (K + GSR_FEAT_CH - 1) / GSR_FEAT_CH; }
size_t gsr_features_valid_offset(int64_t R, int K) { return gsr_align_up((size_t)gsr_features_chunks(K) * (size_t)R * sizeof(float4)); }

void gsr_launch_features_forward(int W, int H, int K, GsrImage img, const uint32_t* point_list, const GsrSplat* splat, const float* features,
                                 float* out, bool cull, hipStream_t s)
{
	const int gx = gsr_grid_x(W), ntiles = gx * gsr_grid_y(H);
	gsr_launch(gsr_features_forward_kernel, dim3((ntiles + GSR_WAVES_PER_WG - 1) / GSR_WAVES_PER_WG, gsr_features_chunks(K)), dim3(64 * GSR_WAVES_PER_WG),
	           0, s, nullptr, nullptr, W, H, gx, ntiles, K, img.ranges, point_list, splat, img.n_contrib, img.tile_max_contrib, features, out,
	           cull ? 1 : 0);
}

void gsr_launch_features_backward_tiles(int W, int H, int K, int64_t R, GsrImage img, const uint32_t* point_list, const GsrSplat* splat,
                                        const uint32_t* slot_base, const float* features, const float* dL_dout, void* scratch,
                                        GsrGradSlot* slots, bool cull, hipStream_t s)
{
	const int gx = gsr_grid_x(W), ntiles = gx * gsr_grid_y(H), nchunks = gsr_features_chunks(K);
	const dim3 grid((ntiles + GSR_WAVES_PER_WG - 1) / GSR_WAVES_PER_WG), block(64 * GSR_WAVES_PER_WG);
	float4* frec = (float4*)scratch;
	uint8_t* fvalid = (uint8_t*)scratch + gsr_features_valid_offset(R, K);
	if (slots) {
		// one chunk per launch: the chunks' additions into the slots happen in launch order
		for (int c = 0; c < nchunks; c++)
			gsr_launch(gsr_features_backward_kernel<true>, grid, block, 0, s, nullptr, nullptr, W, H, gx, ntiles, K, c, (uint32_t)R, img.ranges,
			           point_list, splat, slot_base, img.final_T, img.n_contrib, img.tile_max_contrib, features, dL_dout, frec, fvalid, slots,
			           cull ? 1 : 0);
	} else {
		gsr_launch(gsr_features_backward_kernel<false>, dim3(grid.x, nchunks), block, 0, s, nullptr, nullptr, W, H, gx, ntiles, K, 0, (uint32_t)R,
		           img.ranges, point_list, splat, slot_base, img.final_T, img.n_contrib, img.tile_max_contrib, features, dL_dout, frec, fvalid,
		           (GsrGradSlot*)nullptr, cull ? 1 : 0);
	}
}

void gsr_launch_features_fold(int P, int K, int64_t R, GsrGeometry g, const void* scratch, float* dL_dfeatures, hipStream_t s)
{
	gsr_launch(gsr_features_fold_kernel, dim3((P + 255) / 256), dim3(256), 0, s, nullptr, nullptr, P, K, (uint32_t)R, g.tiles_touched, g.slot_base,
	           (const float4*)scratch, (const uint8_t*)scratch + gsr_features_valid_offset(R, K), dL_dfeatures);
}
