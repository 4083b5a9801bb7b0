// features.hip -- K per-Gaussian feature channels blended with the colour pass's own weights, and their gradients
// (include/gsr_features.h): F_k(p) = sum_i f_ik alpha_i T_i(p), no background term.  Three kernels, no atomics, no workgroup
// barrier, bitwise reproducible.  None of the default kernels is touched: the passes below read the state a forward of any variant
// left, the way contrib.hip does.
//
// Both tile passes are the replay walk of gsr_replay.h.  The channels are processed in chunks of GSR_FEAT_CH = 4 -- 16 accumulators
// per lane -- a ragged last chunk is padded with zero features and zero gradients inside the kernels.  A chunk is one wave's whole walk:
//   forward         grid (tiles, chunks): the chunks of one tile are independent waves of one launch;
//   backward tiles  into_slots = 0: grid (tiles, chunks) as the forward; into_slots = 1: one launch per chunk, in chunk order on the
//                   stream, because every chunk adds into the same six words of the gradient slot (see below) -- the order of these
//                   additions is the launch order, so the sum is reproducible.
//
// Forward tile pass: front to back; w = alpha T has the colour pass's bits and F_k = fma(f_ik, w, F_k), in list order, is what the
// colour kernel would have accumulated for a colour f_ik.  out[K][H][W] is written in full (zeros where nothing blends).
//
// Backward tile pass: backward.cu:507-599 per pixel with the chunk's four channels in place of the three colours and a zero
// background: back to front, accum_rec per channel, the straight-through 0.99 clamp,
// dL/dalpha_i = sum_k (f_ik - accum_rec_k) g_k T_i with g = dL/dF.
// Per (Gaussian, tile) instance with at least one hit the wave reduces (gsr_row_reduce: 4 values, or 10 with SLOTS)
//   (a) the four sums over the pixels of alpha T g_k -- dL/df_ik of this tile -- into the instance's own 16-byte record of the
//       features scratch (chunk c, slot s: record c * R + s; slot numbering of the gradient slots, render_backward.hip), and sets the
//       slot's validity byte (one byte per slot behind the records; the chunks of a call hit the same instances, so they share it);
//   (b) SLOTS only: the raw moments of f = G dL/dG and sum G dL/dalpha (gsr_pair_moments), finished and ADDED into words 0..5 of
//       the GsrGradSlot the colour blend wrote for the same instance (gsr_slot_add_geometry).  Words 6..11 are not touched.  The hit
//       set is the colour blend's, so exactly the slots it validated are updated and the unchanged per-Gaussian backward chains
//       the total.
// Every reduced instance is finished on its own: neither parking (contrib.hip's flush) nor the 64 x 9 transpose is used -- with
// ten values the four-instance flush would not fit 64 lanes.  The launch's tail is the longest list of the view.
//
// Per-Gaussian fold: one lane per Gaussian adds its run of feature records [slot_base[g], + tiles_touched[g]) in index order, chunk
// by chunk, and writes all K elements of dL_dfeatures[g] (zeros without a hit: the caller's memory may be uninitialised).
//
// Registers (hipcc 7.x, gfx950, -O3 -ffp-contract=off; `make audit`, .audit/features.s):
//   gsr_features_forward_kernel             80 VGPRs, 6 waves per SIMD, no scratch
//   gsr_features_backward_kernel<false>     96 VGPRs, 5 waves per SIMD, no scratch
//   gsr_features_backward_kernel<true>     124 VGPRs, 4 waves per SIMD, no scratch
//   gsr_features_fold_kernel                16 VGPRs, 8 waves per SIMD, no scratch
// No kernel spills to scratch (ScratchSize 0, private_segment_fixed_size 0 for all four).
// LDS per wave: forward 3 328 bytes, backward 8 448 bytes (20 waves of the backward: 165 KB -- a CU's 160 KB hold 19, so the
// <false> instantiation is bound by LDS at 19 waves per CU just below its register limit; <true> runs its 16).
#include "gsr_replay.h"

#define GSR_FEAT_CH 4
#define GSR_FEAT_ROWS 16    // rows of the reduction area: lane 4 v + q reads row v, v = 0..15, whatever NV is

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

// the payload of both tile passes: the chunk's four features, staged beside the record
struct GsrFeatStage : GsrReplayPass {
	const float* __restrict__ features;
	int K, ch0;
	float4* feat;   // the wave's 64 staged payloads
	__device__ __forceinline__ float4 load(uint32_t id, const float4*) const { return gsr_feat_load(features, id, K, ch0); }
	__device__ __forceinline__ float put(int pos, const float4& f) const { feat[pos] = f; return 0.f; }
};

struct GsrFeatForwardPass : GsrFeatStage {
	float F[GSR_PIX_PER_LANE][GSR_FEAT_CH];
	__device__ __forceinline__ float4 begin(const GsrInstance& in) const { return feat[in.j]; }
	__device__ __forceinline__ void pixel(const GsrTileWalk&, const GsrInstance&, int k, float, const GsrPairFwd& p, const float4& Fj)
	{
		F[k][0] = __builtin_fmaf(Fj.x, p.w, F[k][0]);
		F[k][1] = __builtin_fmaf(Fj.y, p.w, F[k][1]);
		F[k][2] = __builtin_fmaf(Fj.z, p.w, F[k][2]);
		F[k][3] = __builtin_fmaf(Fj.w, p.w, F[k][3]);
	}
};

__global__ void __launch_bounds__(64 * GSR_WAVES_PER_WG) gsr_features_forward_kernel(
	int W, int H, int gx, int ntiles, int K, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
	const GsrSplat* __restrict__ splat, const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max_contrib,
	const float* __restrict__ features, float* __restrict__ out, int cull)
{
	__shared__ GsrBatchLds s_batch[GSR_WAVES_PER_WG];
	__shared__ float4 s_feat[GSR_WAVES_PER_WG][64];
	GsrTileWalk w;
	gsr_walk_tile(w, gx);
	if (w.tile >= ntiles) return;
	gsr_walk_list(w, ranges, point_list, tile_max_contrib);   // n = 0: the tile's pixels get zeros
	GsrFeatForwardPass pass;
	pass.features = features;
	pass.K = K;
	pass.ch0 = GSR_FEAT_CH * (int)blockIdx.y;
	pass.feat = s_feat[w.wave];
	gsr_walk_pixels<uint32_t>(w, W, H, n_contrib, nullptr, [&](int k, bool, uint32_t) {
#pragma unroll
		for (int c = 0; c < GSR_FEAT_CH; c++) pass.F[k][c] = 0.f;
	});
	GSR_REPLAY(false, false, w, s_batch[w.wave], splat, (const uint32_t*)nullptr, cull, pass);

	const size_t plane = (size_t)H * W;
#pragma unroll
	for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
		if (w.px < W && w.py(k) < H) {
			const size_t pix_id = (size_t)W * w.py(k) + w.px;
#pragma unroll
			for (int c = 0; c < GSR_FEAT_CH; c++)
				if (pass.ch0 + c < K) out[(size_t)(pass.ch0 + c) * plane + pix_id] = pass.F[k][c];
		}
	}
}

template <bool SLOTS>
struct GsrFeatBackwardPass : GsrFeatStage {
	static constexpr int NV = SLOTS ? GSR_FEAT_CH + 6 : GSR_FEAT_CH;
	struct Acc {
		float f[GSR_FEAT_CH];     // the instance's features
		// per-lane partial sums over its four pixels: [0..3] alpha T g_k; SLOTS: [4..8] the raw moments of f = G dL/dG, [9] G dL/dalpha
		float v[NV];
		unsigned long long any;   // lanes with a hit
	};
	float ar[GSR_PIX_PER_LANE][GSR_FEAT_CH];   // accum_rec as the NEXT hit will see it
	float g[GSR_PIX_PER_LANE][GSR_FEAT_CH];    // dL/dF of the pixel
	float* red;                                // the wave's reduction area
	float4* __restrict__ frec;                 // this chunk's records
	uint8_t* __restrict__ fvalid;
	GsrGradSlot* slots;
	float half_w, half_h;

	__device__ __forceinline__ Acc begin(const GsrInstance& in) const
	{
		const float4 Fj = feat[in.j];
		Acc a = {{Fj.x, Fj.y, Fj.z, Fj.w}, {}, 0ull};
		return a;
	}
	__device__ __forceinline__ void pixel(const GsrTileWalk&, const GsrInstance& in, int k, float dy, const GsrPairBwd& p, Acc& a)
	{
		a.any |= p.hitm;
		// dL/dalpha = sum_c (f_c - accum_rec_c) g_c T: the differences first, as the reference forms them, then an FMA chain
		float d[GSR_FEAT_CH];
#pragma unroll
		for (int c = 0; c < GSR_FEAT_CH; c++) d[c] = a.f[c] - ar[k][c];
		float dla = d[0] * g[k][0];
#pragma unroll
		for (int c = 1; c < GSR_FEAT_CH; c++) dla = __builtin_fmaf(d[c], g[k][c], dla);
		// accum_rec' = alpha f + (1 - alpha) accum_rec, on the difference above (render_backward.hip)
#pragma unroll
		for (int c = 0; c < GSR_FEAT_CH; c++) ar[k][c] = __builtin_fmaf(p.alpha, d[c], ar[k][c]);
		dla = p.hit ? dla * p.Tn : 0.f;   // (zero background: no T_final term)
		const float dch = p.alpha * p.Tn;  // dF/df; 0 without a hit
#pragma unroll
		for (int c = 0; c < GSR_FEAT_CH; c++) a.v[c] = __builtin_fmaf(dch, g[k][c], a.v[c]);
		if constexpr (SLOTS) gsr_pair_moments(a.v + 4, a.v[9], in.B.y, p.G, dla, in.dx, dy);
	}
	__device__ __forceinline__ void finish(const GsrTileWalk& w, const GsrInstance& in, Acc& a) const
	{
		if (a.any == 0ull) return;   // wave-uniform: nothing is written for an instance without a hit
		float S[NV];   // wave-uniform
		gsr_row_reduce<NV, GSR_FEAT_ROWS>(red, w.lane, a.v, S);
		const uint32_t slot = in.slot();
		if (w.lane == 0) {
			frec[slot] = make_float4(S[0], S[1], S[2], S[3]);
			fvalid[slot] = 1;
		}
		if constexpr (SLOTS) gsr_slot_add_geometry(slots, slot, w.lane, in, half_w, half_h, S + 4, S[9]);
	}
};

// SLOTS: also the six geometry quantities, added into words 0..5 of the instance's gradient slot (grid.y must be 1: one chunk per launch)
template <bool SLOTS>
__global__ void __launch_bounds__(64 * GSR_WAVES_PER_WG) gsr_features_backward_kernel(
	int W, int H, int gx, int ntiles, int K, int chunk0, uint32_t R, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
	const GsrSplat* __restrict__ splat, const uint32_t* __restrict__ slot_base, const float* __restrict__ final_Ts,
	const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max_contrib, const float* __restrict__ features,
	const float* __restrict__ dL_dout, float4* __restrict__ frec, uint8_t* __restrict__ fvalid, GsrGradSlot* slots, int cull)
{
	__shared__ GsrBatchLds s_batch[GSR_WAVES_PER_WG];
	__shared__ float4 s_feat[GSR_WAVES_PER_WG][64];
	__shared__ __attribute__((aligned(16))) float s_red[GSR_WAVES_PER_WG][GSR_FEAT_ROWS * GSR_REPLAY_ROW];
	GsrTileWalk w;
	gsr_walk_tile(w, gx);
	if (w.tile >= ntiles) return;
	gsr_walk_list(w, ranges, point_list, tile_max_contrib);
	if (w.n <= 0) return;

	const int chunk = chunk0 + (int)blockIdx.y;
	GsrFeatBackwardPass<SLOTS> pass;
	pass.features = features;
	pass.K = K;
	pass.ch0 = GSR_FEAT_CH * chunk;
	pass.feat = s_feat[w.wave];
	pass.red = s_red[w.wave];
	pass.frec = frec + (size_t)chunk * R;
	pass.fvalid = fvalid;
	pass.slots = slots;
	pass.half_w = 0.5f * W;
	pass.half_h = 0.5f * H;
	const size_t plane = (size_t)H * W;
	gsr_walk_pixels<size_t>(w, W, H, n_contrib, final_Ts, [&](int k, bool inside, size_t pix_id) {
#pragma unroll
		for (int c = 0; c < GSR_FEAT_CH; c++) {
			pass.ar[k][c] = 0.f;
			pass.g[k][c] = (inside && pass.ch0 + c < K) ? dL_dout[(size_t)(pass.ch0 + c) * plane + pix_id] : 0.f;
		}
	});
	GSR_REPLAY(true, true, w, s_batch[w.wave], splat, slot_base, cull, pass);
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

void gsr_launch_features_forward(const GsrFrame& f, int K, const float* features, float* out)
{
	const GsrTileGrid t = gsr_tile_grid(f.W, f.H, gsr_features_chunks(K));
	gsr_launch(gsr_features_forward_kernel, t.grid, t.block, 0, f.s, nullptr, nullptr, f.W, f.H, t.gx, t.ntiles, K, f.img.ranges, f.bin.point_list,
	           f.g.splat, f.img.n_contrib, f.img.tile_max_contrib, features, out, f.cull ? 1 : 0);
}

void gsr_launch_features_backward_tiles(const GsrFrame& f, int K, const float* features, const float* dL_dout, void* scratch)
{
	const int nchunks = gsr_features_chunks(K);
	const GsrTileGrid t = gsr_tile_grid(f.W, f.H);
	const GsrImage& img = f.img;
	float4* frec = (float4*)scratch;
	uint8_t* fvalid = (uint8_t*)scratch + gsr_features_valid_offset(f.R, K);
	if (f.slots) {
		// one chunk per launch: the chunks' additions into the slots happen in launch order
		for (int c = 0; c < nchunks; c++)
			gsr_launch(gsr_features_backward_kernel<true>, t.grid, t.block, 0, f.s, nullptr, nullptr, f.W, f.H, t.gx, t.ntiles, K, c, (uint32_t)f.R, img.ranges,
			           f.bin.point_list, f.g.splat, f.g.slot_base, img.final_T, img.n_contrib, img.tile_max_contrib, features, dL_dout, frec, fvalid,
			           f.slots, f.cull ? 1 : 0);
	} else {
		gsr_launch(gsr_features_backward_kernel<false>, dim3(t.grid.x, nchunks), t.block, 0, f.s, nullptr, nullptr, f.W, f.H, t.gx, t.ntiles, K, 0,
		           (uint32_t)f.R, img.ranges, f.bin.point_list, f.g.splat, f.g.slot_base, img.final_T, img.n_contrib, img.tile_max_contrib, features, dL_dout,
		           frec, fvalid, (GsrGradSlot*)nullptr, f.cull ? 1 : 0);
	}
}

void gsr_launch_features_fold(const GsrFrame& f, int K, const void* scratch, float* dL_dfeatures)
{
	gsr_launch(gsr_features_fold_kernel, dim3((f.P + 255) / 256), dim3(256), 0, f.s, nullptr, nullptr, f.P, K, (uint32_t)f.R, f.g.tiles_touched,
	           f.g.slot_base, (const float4*)scratch, (const uint8_t*)scratch + gsr_features_valid_offset(f.R, K), dL_dfeatures);
}
