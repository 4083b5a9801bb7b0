// gsr_replay.h -- the tile-list replay walk, once.  The passes that run after a forward and read the state it left (contrib.hip,
// features.hip, distortion.hip, median.hip) all walk a tile's list the way the colour pass did; this header holds that walk and
// each pass supplies only what is particular to it (DESIGN.md "Replay walk").
//
// Decomposition (render_common.h): one wave64 per 16x16 tile, four pixels per lane.  The walk covers the list positions
// [0, n), n = min(range length, tile_max_contrib) -- the tail was never blended -- and for a pixel only the positions in front of its
// n_contrib, front to back, or back to front from final_T (T_i = T_{i+1} / (1 - alpha_i), v_rcp_f32 as render_backward.hip).
// `power`, alpha, the two thresholds and T's update are render_forward.hip's instruction sequence on the same records
// (gsr_pair_power_halved, __expf, fminf(0.99, .), __fmul_rn, __fsub_rn): every w = alpha T has the colour pass's bits and no
// accept / reject decision differs, so the hit set of a replay is the colour blend's.  tile_order is not read (tiles are taken in
// index order), nothing of the forward's state is written, heavy tiles are walked whole by one wave (no depth segments), and there
// is no workgroup barrier and no atomic anywhere: a wave's LDS operations execute in program order, the wave barriers only keep
// the compiler from moving LDS accesses across them.
//
// A kernel is: gsr_walk_tile / gsr_walk_list / gsr_walk_pixels (with its two early exits between them), a pass object, GSR_REPLAY,
// and its own output stores.  A pass is a struct derived from GsrReplayPass that holds its per-pixel state (register arrays indexed by the pixel slot k; every
// hook is inlined, so they stay in registers) and overrides the hooks it needs:
//   load(id, p)             a per-instance payload gathered next to the splat record p of Gaussian id, one batch ahead
//   put(pos, payload)       stores the payload of a surviving instance into LDS the pass owns; returns the word that rides in
//                           rec[1].w when the walk carries no slot address there
//   begin(in)               the per-instance accumulator, created once per staged instance
//   pixel(w, in, k, dy, p, a)  one (instance, pixel slot) pair with at least one hit in the wave; p: GsrPairFwd or GsrPairBwd
//   finish(w, in, a)        after the four pixel slots: reduce and store
//   batch_done(w, next)     after a batch, every position below `next` walked; false ends the walk
#pragma once
#include "render_common.h"

#define GSR_REPLAY_ROW 80   // words between two rows of a reduction area: the rows of one 8-lane read group then sit 16 banks apart

// the surviving instances of a batch: (x, y, -0.5 conic a, conic b), (-0.5 conic c, opacity, list position, slot or put()'s word),
// and the band mask
struct GsrBatchLds {
	float4 rec[2][64];
	uint32_t bands[64];
};

struct GsrTileWalk {
	int wave, lane, tile, tx, ty, px, py0;
	float pfx, x0f, y0f;
	int n;                                  // min(range length, tile_max_contrib)
	const uint32_t* plist;
	float T[GSR_PIX_PER_LANE];              // the pixel's transmittance at the walk's current position
	float pfy[GSR_PIX_PER_LANE];
	uint32_t last[GSR_PIX_PER_LANE];        // the pixel's n_contrib: it blended positions in front of this one only (0 outside the image)
	uint32_t band_last[GSR_PIX_PER_LANE];   // wave-uniform: the largest of them in band k
	__device__ __forceinline__ int py(int k) const { return py0 + 4 * k; }
};

// The set-up comes in three steps with the kernel's two early exits between them, `if (w.tile >= ntiles) return;` and, where an
// empty walk leaves nothing to write, `if (w.n <= 0) return;` (both wave-uniform; a replay kernel has no workgroup barrier).  The
// exits stay in the kernel: an exit flag handed back by a function is a second branch the compiler does not fold on this target.
__device__ __forceinline__ void gsr_walk_tile(GsrTileWalk& w, int gx)
{
	w.wave = threadIdx.x >> 6;
	w.lane = threadIdx.x & 63;
	w.tile = blockIdx.x * GSR_WAVES_PER_WG + w.wave;
	w.tx = w.tile % gx;
	w.ty = w.tile / gx;
	w.px = w.tx * GSR_TILE_X + (w.lane & 15);
	w.py0 = w.ty * GSR_TILE_Y + (w.lane >> 4);
	w.pfx = (float)w.px;
	w.x0f = (float)(w.tx * GSR_TILE_X);
	w.y0f = (float)(w.ty * GSR_TILE_Y);
}

__device__ __forceinline__ void gsr_walk_list(GsrTileWalk& w, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                                              const uint32_t* __restrict__ tile_max_contrib)
{
	const uint2 range = ranges[w.tile];
	w.n = (int)min(range.y - range.x, tile_max_contrib[w.tile]);  // the tail was never blended
	w.plist = point_list + range.x;
}

// final_T: NULL for a front-to-back walk (T starts at 1), the forward's final_T plane for a back-to-front one.  pixel_init(k, inside,
// pix_id) loads the pass's own per-pixel state next to the walk's.
template <class Index, class PixelInit>
__device__ __forceinline__ void gsr_walk_pixels(GsrTileWalk& w, int W, int H, const uint32_t* __restrict__ n_contrib, const float* __restrict__ final_T,
                                                PixelInit&& pixel_init)
{
#pragma unroll
	for (int k = 0; k < GSR_PIX_PER_LANE; k++) {
		const int py = w.py(k);
		const bool inside = w.px < W && py < H;
		const Index pix_id = inside ? (Index)W * py + w.px : 0;
		w.pfy[k] = (float)py;
		w.T[k] = final_T ? (inside ? final_T[pix_id] : 0.f) : 1.0f;
		w.last[k] = inside ? n_contrib[pix_id] : 0u;
		pixel_init(k, inside, pix_id);
		uint32_t m = w.last[k];
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
		w.band_last[k] = __builtin_amdgcn_readfirstlane(m);
	}
}

// the gradient-slot numbering of render_backward.hip: one slot per (Gaussian, tile of its trimmed rect)
__device__ __forceinline__ uint32_t gsr_slot_index(uint32_t sbase, uint32_t rect_min, uint32_t rect_wh, int tx, int ty)
{
	return sbase + ((uint32_t)ty - (rect_min >> 16)) * (rect_wh & 0xffffu) + ((uint32_t)tx - (rect_min & 0xffffu));
}

// one staged instance, as every lane reads it back
struct GsrInstance {
	float4 A;            // x, y, -0.5 conic a, conic b
	float4 B;            // -0.5 conic c, opacity, list position, slot or put()'s word
	uint32_t position;   // wave-uniform (backward.cu:511-515)
	float dx, ax2, bdx;  // shared by the lane's four pixels
	int j;               // its place in the batch's LDS arrays
	__device__ __forceinline__ uint32_t slot() const { return __builtin_amdgcn_readfirstlane(__float_as_uint(B.w)); }
};

// ---- pair evaluation: the colour passes' instruction sequences.  `body` runs where at least one lane hits (wave-uniform) ----
struct GsrPairFwd {
	unsigned long long hitm;   // lanes that blend
	bool hit;
	float w;                   // the forward's alpha * T; 0 without a hit
	float Tfront;              // T in front of the instance
};

template <class Body>
__device__ __forceinline__ void gsr_pair_forward(const GsrInstance& in, float dy, uint32_t last, float& T, Body&& body)
{
	const float power = gsr_pair_power_halved(in.ax2, in.bdx, in.B.x, dy);
	const float alpha = fminf(0.99f, in.B.y * __expf(power));
	GsrPairFwd p;
	p.hitm = __builtin_amdgcn_ballot_w64(in.position < last) & __builtin_amdgcn_ballot_w64(!(power > 0.0f)) &
	         __builtin_amdgcn_ballot_w64(!(alpha < 1.0f / 255.0f));
	if (p.hitm == 0ull) return;  // wave-uniform
	p.hit = __builtin_amdgcn_inverse_ballot_w64(p.hitm);
	p.Tfront = T;
	p.w = p.hit ? __fmul_rn(alpha, T) : 0.0f;
	T = p.hit ? __fmul_rn(T, __fsub_rn(1.0f, alpha)) : T;   // the forward's T (1 - alpha), rounded as there
	body(p);
}

struct GsrPairBwd {
	unsigned long long hitm;   // lanes that blended
	bool hit;
	float G;                   // exp(power)
	float alpha;               // clamped; 0 without a hit: the pixel runs the same update as the identity on its state, bit for bit
	float Tn;                  // T in front of the instance (T is set to it)
};

template <class Body>
__device__ __forceinline__ void gsr_pair_backward(const GsrInstance& in, float dy, uint32_t last, float& T, Body&& body)
{
	const float power = gsr_pair_power_halved(in.ax2, in.bdx, in.B.x, dy);
	GsrPairBwd p;
	p.G = __expf(power);
	const float araw = fminf(0.99f, in.B.y * p.G);
	p.hitm = __builtin_amdgcn_ballot_w64(in.position < last) & __builtin_amdgcn_ballot_w64(!(power > 0.0f)) &
	         __builtin_amdgcn_ballot_w64(!(araw < 1.0f / 255.0f));
	if (p.hitm == 0ull) return;  // wave-uniform
	p.hit = __builtin_amdgcn_inverse_ballot_w64(p.hitm);
	p.alpha = p.hit ? araw : 0.f;
	p.Tn = T * __builtin_amdgcn_rcpf(1.f - p.alpha);
	T = p.Tn;
	body(p);
}

// the form of the walk's direction
template <bool BACK, class Body>
__device__ __forceinline__ void gsr_pair(const GsrInstance& in, float dy, uint32_t last, float& T, Body&& body)
{
	if constexpr (BACK) gsr_pair_backward(in, dy, last, T, body);
	else gsr_pair_forward(in, dy, last, T, body);
}

// the raw moments of f = G dL/dG over a lane's pixels, added pair by pair: M[0..4] = sum f dx, f dy, f dx^2, f dx dy, f dy^2 and
// dop = sum G dL/dalpha; `opacity` is the record's, dla the pair's dL/dalpha (straight through the 0.99 clamp)
__device__ __forceinline__ void gsr_pair_moments(float* M, float& dop, float opacity, float G, float dla, float dx, float dy)
{
	dop = __builtin_fmaf(G, dla, dop);
	const float f = (opacity * dla) * G;
	const float fdx = f * dx, fdy = f * dy;
	M[0] += fdx;
	M[1] += fdy;
	M[2] = __builtin_fmaf(fdx, dx, M[2]);
	M[3] = __builtin_fmaf(fdx, dy, M[3]);
	M[4] = __builtin_fmaf(fdy, dy, M[4]);
}

// the hooks a pass does not need
struct GsrReplayPass {
	struct None {};
	__device__ __forceinline__ None load(uint32_t, const float4*) const { return None{}; }
	template <class P> __device__ __forceinline__ float put(int, const P&) const { return 0.f; }
	__device__ __forceinline__ None begin(const GsrInstance&) const { return None{}; }
	template <class A> __device__ __forceinline__ void finish(const GsrTileWalk&, const GsrInstance&, A&) const {}
	__device__ __forceinline__ bool batch_done(GsrTileWalk&, uint32_t) const { return true; }
};

// The walk.  BACK_: back to front, batch position q maps to list position n - 1 - q.  SLOT_: rec[1].w carries the instance's slot
// address (slot_base_ is read).  Software pipeline: records and payloads one batch ahead, ids two batches ahead; the instances of a
// batch that gsr_tile_band_mask leaves (cull_) are compacted into the wave's LDS slice lds_, the conic's a and c pre-multiplied by
// -0.5 (exact), and then read back one at a time by the whole wave: per pixel slot a scalar branch skips a band the instance cannot
// reach or none of whose pixels blended this far (or that has finished: median.hip), and the pair is evaluated.
//
// A statement macro, expanded once in each kernel, and not a function template: as a function -- inlined by force or by the
// optimiser's choice -- the same text compiled to front-to-back kernels that carry the pass's accumulators twice through the batch
// loop (features forward 98 instead of 84 VGPRs, 4 instead of 5 waves per SIMD; distortion forward 98 instead of 84; both median
// twins 94).  Expanded in place the kernels keep the registers, LDS and occupancy of the hand-written walks they replace
// (profiles/replay_refactor_isa.txt).  The price of a macro: its locals carry the prefix gsr_r_ so that an argument expression
// cannot be captured by one of them -- pass no expression that uses such a name -- and a compile error inside it is reported at
// the line of the expansion.
#define GSR_REPLAY(BACK_, SLOT_, w_, lds_, splat_, slot_base_, cull_, pass_)                                                                          \
	do {                                                                                                                                                 \
		const int gsr_r_n = (w_).n, gsr_r_lane = (w_).lane;                                                                                                 \
		float4 gsr_r_ra = make_float4(0, 0, 0, 0), gsr_r_rb = gsr_r_ra;                                                                                     \
		decltype((pass_).load(0u, (const float4*)nullptr)) gsr_r_pay{};                                                                                     \
		uint32_t gsr_r_sbase = 0u;                                                                                                                          \
		auto gsr_r_list_pos = [&](int gsr_r_q) { return (BACK_) ? gsr_r_n - 1 - gsr_r_q : gsr_r_q; };                                                       \
		auto gsr_r_gather = [&](uint32_t gsr_r_id) {                                                                                                        \
			const float4* gsr_r_p = reinterpret_cast<const float4*>((splat_) + gsr_r_id);                                                                      \
			gsr_r_ra = gsr_r_p[0]; gsr_r_rb = gsr_r_p[1];                                                                                                      \
			gsr_r_pay = (pass_).load(gsr_r_id, gsr_r_p);                                                                                                       \
			if ((SLOT_)) gsr_r_sbase = (slot_base_)[gsr_r_id];                                                                                                 \
		};                                                                                                                                                  \
		if (gsr_r_lane < gsr_r_n) gsr_r_gather((w_).plist[gsr_r_list_pos(gsr_r_lane)]);                                                                     \
		uint32_t gsr_r_id_next = (64 + gsr_r_lane < gsr_r_n) ? (w_).plist[gsr_r_list_pos(64 + gsr_r_lane)] : 0u;                                            \
		for (int gsr_r_base = 0; gsr_r_base < gsr_r_n; gsr_r_base += 64) {                                                                                  \
			const uint32_t gsr_r_bands = (gsr_r_base + gsr_r_lane < gsr_r_n) ? ((cull_) ? gsr_tile_band_mask(gsr_r_ra.x, gsr_r_ra.y, gsr_r_ra.z, gsr_r_ra.w, gsr_r_rb.x, gsr_r_rb.y, (w_).x0f, (w_).y0f) : 0xFu) : 0u; \
			const bool gsr_r_keep = gsr_r_bands != 0u;                                                                                                         \
			const unsigned long long gsr_r_mask = __builtin_amdgcn_ballot_w64(gsr_r_keep);                                                                     \
			const int gsr_r_cnt = __popcll(gsr_r_mask);                                                                                                        \
			if (gsr_r_keep) {                                                                                                                                  \
				const int gsr_r_pos = gsr_mbcnt(gsr_r_mask);                                                                                                      \
				float gsr_r_w1 = (pass_).put(gsr_r_pos, gsr_r_pay);                                                                                               \
				if ((SLOT_)) gsr_r_w1 = __uint_as_float(gsr_slot_index(gsr_r_sbase, __float_as_uint(gsr_r_rb.z), __float_as_uint(gsr_r_rb.w), (w_).tx, (w_).ty)); \
				(lds_).rec[0][gsr_r_pos] = make_float4(gsr_r_ra.x, gsr_r_ra.y, -0.5f * gsr_r_ra.z, gsr_r_ra.w);                                                   \
				(lds_).rec[1][gsr_r_pos] = make_float4(-0.5f * gsr_r_rb.x, gsr_r_rb.y, __uint_as_float((uint32_t)gsr_r_list_pos(gsr_r_base + gsr_r_lane)), gsr_r_w1); \
				(lds_).bands[gsr_r_pos] = gsr_r_bands;                                                                                                            \
			}                                                                                                                                                  \
			if (gsr_r_base + 64 + gsr_r_lane < gsr_r_n) gsr_r_gather(gsr_r_id_next);                                                                           \
			gsr_r_id_next = (gsr_r_base + 128 + gsr_r_lane < gsr_r_n) ? (w_).plist[gsr_r_list_pos(gsr_r_base + 128 + gsr_r_lane)] : 0u;                        \
			__builtin_amdgcn_wave_barrier();                                                                                                                   \
			for (int gsr_r_j = 0; gsr_r_j < gsr_r_cnt; gsr_r_j++) {                                                                                            \
				GsrInstance gsr_r_in;                                                                                                                             \
				gsr_r_in.A = (lds_).rec[0][gsr_r_j];                                                                                                              \
				gsr_r_in.B = (lds_).rec[1][gsr_r_j];                                                                                                              \
				gsr_r_in.position = __builtin_amdgcn_readfirstlane(__float_as_uint(gsr_r_in.B.z));                                                                \
				const uint32_t gsr_r_jbands = __builtin_amdgcn_readfirstlane((lds_).bands[gsr_r_j]); /* wave-uniform */                                           \
				gsr_r_in.dx = gsr_r_in.A.x - (w_).pfx;                                                                                                            \
				gsr_r_in.ax2 = __fmul_rn(__fmul_rn(gsr_r_in.A.z, gsr_r_in.dx), gsr_r_in.dx);                                                                      \
				gsr_r_in.bdx = __fmul_rn(gsr_r_in.A.w, gsr_r_in.dx);                                                                                              \
				gsr_r_in.j = gsr_r_j;                                                                                                                             \
				auto gsr_r_acc = (pass_).begin(gsr_r_in);                                                                                                         \
				_Pragma("unroll") for (int gsr_r_k = 0; gsr_r_k < GSR_PIX_PER_LANE; gsr_r_k++) {                                                                  \
					if (!(gsr_r_jbands & (1u << gsr_r_k)) || gsr_r_in.position >= (w_).band_last[gsr_r_k]) continue;                                                 \
					const float gsr_r_dy = gsr_r_in.A.y - (w_).pfy[gsr_r_k];                                                                                         \
					gsr_pair<(BACK_)>(gsr_r_in, gsr_r_dy, (w_).last[gsr_r_k], (w_).T[gsr_r_k], [&](const auto& gsr_r_p) { (pass_).pixel((w_), gsr_r_in, gsr_r_k, gsr_r_dy, gsr_r_p, gsr_r_acc); }); \
				}                                                                                                                                                 \
				(pass_).finish((w_), gsr_r_in, gsr_r_acc);                                                                                                        \
			}                                                                                                                                                  \
			__builtin_amdgcn_wave_barrier();                                                                                                                   \
			if (!(pass_).batch_done((w_), (uint32_t)gsr_r_base + 64u)) break; /* wave-uniform */                                                               \
		}                                                                                                                                                   \
	} while (0)

// The wave reduction of one instance's NV per-lane partials through LDS: each lane stores its partials into NV rows of 64 words
// (`red`: ROWS rows of GSR_REPLAY_ROW words, 16-byte aligned), lane 4 v + q reads the 16 words of quarter q of row v & (ROWS - 1)
// with four ds_read_b128 and folds them, two lane exchanges (ds_bpermute_b32) join the quarters, and the totals are broadcast as
// scalars (v_readlane_b32).  Per instance: NV ds_write_b32, 4 ds_read_b128, 17 adds, 2 ds_bpermute_b32 -- the cross-lane work
// stays on the LDS pipe.  The order of the additions is fixed.
template <int NV, int ROWS>
__device__ __forceinline__ void gsr_row_reduce(float* red, int lane, const float (&acc)[NV], float (&S)[NV])
{
	static_assert(NV <= ROWS && (ROWS == 8 || ROWS == 16), "lane 4 v + q must find its row");
	const float* const red_r = red + ((lane >> 2) & (ROWS - 1)) * GSR_REPLAY_ROW + 16 * (lane & 3);
#pragma unroll
	for (int i = 0; i < NV; i++) red[i * GSR_REPLAY_ROW + lane] = acc[i];
	__builtin_amdgcn_wave_barrier();
	const float4 q0 = *reinterpret_cast<const float4*>(red_r), q1 = *reinterpret_cast<const float4*>(red_r + 4);
	const float4 q2 = *reinterpret_cast<const float4*>(red_r + 8), q3 = *reinterpret_cast<const float4*>(red_r + 12);
	__builtin_amdgcn_wave_barrier();
	float t = (((q0.x + q0.y) + (q0.z + q0.w)) + ((q1.x + q1.y) + (q1.z + q1.w))) + (((q2.x + q2.y) + (q2.z + q2.w)) + ((q3.x + q3.y) + (q3.z + q3.w)));
	t += __shfl_xor(t, 1, 64);
	t += __shfl_xor(t, 2, 64);   // lanes 4 v .. 4 v + 3 hold the wave's total of value v (rows >= NV: never used)
#pragma unroll
	for (int i = 0; i < NV; i++) S[i] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(t), 4 * i));
}

// render_backward.hip's epilogue on the wave totals M[0..4] (gsr_pair_moments) and dop: dL/dmean2D = -0.5 W (a sx + b sy),
// -0.5 H (c sy + b sx), with a = -2 (-0.5 a) inside the FMA; dL/dconic .x .y .w = -0.5 x the second moments; dL/dopacity as it is.
// ADDED into words 0..5 of the GsrGradSlot the colour blend wrote for the same instance: a plain read-modify-write by lanes 0..5 of
// the one wave that owns the tile in this launch.  WORD9: lane 6 adds dv into word 9 (pad0, the aux blend's own dL/dv) in the same
// read-modify-write -- a second one of its own cost distortion.hip's backward 13 % (profiles/replay_refactor_isa.txt).
// half_w = 0.5 W, half_h = 0.5 H.
template <bool WORD9 = false>
__device__ __forceinline__ void gsr_slot_add_geometry(GsrGradSlot* slots, uint32_t slot, int lane, const GsrInstance& in, float half_w, float half_h,
                                                      const float* M, float dop, float dv = 0.f)
{
	const float ca = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(in.A.z)));
	const float cb = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(in.A.w)));
	const float cc = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(in.B.x)));
	const float r0 = -half_w * __builtin_fmaf(-2.0f, ca * M[0], cb * M[1]);
	const float r1 = -half_h * __builtin_fmaf(-2.0f, cc * M[1], cb * M[0]);
	const float last = WORD9 ? (lane == 5 ? dop : dv) : dop;
	const float r = lane == 0 ? r0 : lane == 1 ? r1 : lane == 2 ? -0.5f * M[2] : lane == 3 ? -0.5f * M[3] : lane == 4 ? -0.5f * M[4] : last;
	if (lane < (WORD9 ? 7 : 6)) {
		float* p = reinterpret_cast<float*>(slots + slot) + ((WORD9 && lane == 6) ? 9 : lane);
		*p = *p + r;
	}
}

// host side: one wave per tile
struct GsrTileGrid {
	int gx, ntiles;
	dim3 grid, block;
};
static inline GsrTileGrid gsr_tile_grid(int W, int H, int grid_y = 1)
{
	GsrTileGrid t;
	t.gx = gsr_grid_x(W);
	t.ntiles = t.gx * gsr_grid_y(H);
	t.grid = dim3((t.ntiles + GSR_WAVES_PER_WG - 1) / GSR_WAVES_PER_WG, grid_y);
	t.block = dim3(64 * GSR_WAVES_PER_WG);
	return t;
}
