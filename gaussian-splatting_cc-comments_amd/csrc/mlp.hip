// mlp.hip -- a fully fused small MLP on the fp32-input matrix cores with an optional frequency encoding (include/gsr_mlp.h, which
// holds the rule; compiled with -ffp-contract=off, every fma outside the MFMA is written out).
//
// v_mfma_f32_32x32x2_f32 computes D[i][j] = fmaf(A[i][1], B[1][j], fmaf(A[i][0], B[0][j], C[i][j])), a k-ordered fp32 fmaf chain
// (vq.hip).  Lane l holds A[l & 31][l >> 5] and B[l >> 5][l & 31]; of the result it holds column l & 31 and the rows
// (r & 3) + 8 (r >> 2) + 4 (l >> 5), r = 0 .. 15.  Data rows are the columns j throughout: a wave owns 32 rows of the tile, a lane one
// of them, and a layer is NT accumulators of sixteen neurons each, started at the bias.  NT = ceil(widest layer / 32) is the
// instantiation's, the same for all its layers: with a count per layer every MFMA sat behind a branch of its own, and the register
// allocator paid for it with whole copies of the accumulators (scratch at NT = 4).
//   * A pre-pass of weights-only size writes, per layer, the forward image Wt[k][o] (transposed, the operand A of z = W a), the
//     backward image Wb[o][k] (the operand A of da = W^T dz) and the bias, zero-padded: k to the instruction's step of two, the
//     other index to P = 32 NT.  A row of an image is (P | 32) floats, so that the two lane halves of an operand read
//     (rows k and k + 1) fall on different halves of the 64 banks.  An image is one straight 16-byte copy into the LDS, shared by the
//     workgroup's waves and staged layer by layer.
//   * Activations stay in the LDS, a[wave][k][row], a k row being wrows + 1 floats: written from the accumulator layout (a lane writes
//     its own column), read back as the next layer's B operand B[k = 2 s + half][row], and, for dW, read across: dW's MFMA has the
//     row as its k dimension, A = dz[o][row], B = a[k][row].  Padded neurons and rows past N are stored as +0, so a NaN or inf in
//     one row never meets a padding weight or another row.
//   * forward: in place in one buffer per wave.  backward: a persistent workgroup takes the tiles g, g + G, ..; per tile it
//     recomputes the forward keeping a_0 .. a_{M-1}, turns z_M into dz_M, and walks down: the 32 x 32 blocks of dW_l
//     are dealt to the waves, and a block's owner chains over all the tile's rows in ascending order on top of the workgroup's
//     partial in global memory (read and written by the same lane: plain loads and stores); db_l has a lane per neuron; then every
//     wave forms da_{l-1} for its own rows.  gsr_mlp_fold_kernel adds the partials in ascending workgroup order.
// Tile rows R of the backward (gsr_mlp_tile_rows): the largest of 128, 64, 32 whose M + 1 buffers and largest image fit the 160 KB of
// LDS, and 16 (one wave, half its columns idle, k rows of 17 floats) where 32 do not: 5 x 128.  The forward takes 256 rows, 128 at
// NT = 4.  DESIGN.md 6z has the table of registers and LDS per instantiation.
#include "gsr_internal.h"
#include "gsr_depth_key.h"
#include "../../include/gsr_mlp.h"

#include <math.h>

#include <algorithm>

#define GSR_MLP_LDS_BYTES (160 * 1024)
#define GSR_MLP_SLACK 32   // floats behind the last buffer: lanes past a 16-row wave's columns read there

typedef float gsr_f32x16 __attribute__((ext_vector_type(16)));

struct GsrMlpParams {
	int N, M, D, L, hidden, outact, x_planes, y_planes;
	int P;                        // the padded width of every layer: 32 NT
	int waves, wrows;             // waves per workgroup, rows per wave (32, or 16 with a single wave)
	int G, ntiles;                // backward: workgroups, tiles of waves * wrows rows
	int d[GSR_MLP_MAX_LAYERS + 1];
	long long xs, ys, dys, dxs;
	const float* x;
	float* y;
	const float* dy;
	float* dx;
	const float* prep;            // the images
	int wt_off[GSR_MLP_MAX_LAYERS], wb_off[GSR_MLP_MAX_LAYERS], bias_off[GSR_MLP_MAX_LAYERS];   // float offsets into prep, layer l at [l - 1]
	int img_floats;               // the largest image
	float* part;                  // [G][part_stride] partials of dW and db
	long long part_stride;
	int pw_off[GSR_MLP_MAX_LAYERS], pb_off[GSR_MLP_MAX_LAYERS];
	unsigned want_w, want_b;      // bit l - 1: dW_l / db_l is formed
	int want_dx;
};
struct GsrMlpWeights {
	const float* W[GSR_MLP_MAX_LAYERS];
	const float* b[GSR_MLP_MAX_LAYERS];
};
struct GsrMlpGrads {
	float* dW[GSR_MLP_MAX_LAYERS];
	float* db[GSR_MLP_MAX_LAYERS];
};

static __host__ __device__ inline int gsr_mlp_pad32(int d) { return (d + 31) & ~31; }
static __host__ __device__ inline int gsr_mlp_pad2(int d) { return (d + 1) & ~1; }
static __host__ __device__ constexpr int gsr_mlp_stride(int p) { return p | 32; }

// ---- the pre-pass: blockIdx.y = layer - 1 ----
__global__ void __launch_bounds__(256) gsr_mlp_prepare_kernel(GsrMlpParams p, GsrMlpWeights w, float* __restrict__ prep)
{
	const int l = blockIdx.y + 1, dout = p.d[l], din = p.d[l - 1];
	const float* __restrict__ W = w.W[l - 1];
	const float* __restrict__ b = w.b[l - 1];
	const int st = gsr_mlp_stride(p.P), nt = gsr_mlp_pad2(din) * st;
	const int sb = st, nb = gsr_mlp_pad2(dout) * sb;
	const int nbias = p.P;
	for (int e = blockIdx.x * 256 + threadIdx.x; e < nt + nb + nbias; e += gridDim.x * 256) {
		if (e < nt) {
			const int k = e / st, o = e % st;
			prep[p.wt_off[l - 1] + e] = (k < din && o < dout) ? W[(size_t)o * din + k] : 0.f;
		} else if (e < nt + nb) {
			const int o = (e - nt) / sb, k = (e - nt) % sb;
			prep[p.wb_off[l - 1] + (e - nt)] = (k < din && o < dout) ? W[(size_t)o * din + k] : 0.f;
		} else {
			const int o = e - nt - nb;
			prep[p.bias_off[l - 1] + o] = (b && o < dout) ? b[o] : 0.f;
		}
	}
}

// ---- pieces shared by the two kernels ----
__device__ __forceinline__ int gsr_mlp_neuron(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// `floats` floats (a multiple of 4) from global memory into the LDS, by the whole workgroup
__device__ __forceinline__ void gsr_mlp_stage(float* dst, const float* __restrict__ src, int floats)
{
	for (int e = threadIdx.x; e < floats / 4; e += blockDim.x) ((float4*)dst)[e] = ((const float4*)src)[e];
}

// the tile's input rows, encoded, as a_0[wave][k][row]; rows past N are +0 throughout, and so are the k rows d_0 .. P - 1: the one
// that pads d_0 to the instruction's step, and those that dW_1's last block of 32 columns reads beside the real ones
__device__ __forceinline__ void gsr_mlp_load_input(const GsrMlpParams& p, long long row0, int rows, float* a0, int wave_floats, int as)
{
	const int d0 = p.d[0];
	const int padf = wave_floats - d0 * as;   // floats behind the real k rows of one wave's buffer
	for (int e = threadIdx.x; e < p.waves * padf; e += blockDim.x) a0[(e / padf) * wave_floats + d0 * as + e % padf] = 0.f;
	for (int e = threadIdx.x; e < rows * p.D; e += blockDim.x) {
		const int r = p.x_planes ? e % rows : e / p.D, c = p.x_planes ? e / rows : e % p.D;
		const long long row = row0 + r;
		const bool valid = row < p.N;
		const float v = valid ? (p.x_planes ? p.x[(size_t)c * p.xs + row] : p.x[(size_t)row * p.xs + c]) : 0.f;
		float* dst = a0 + (r / p.wrows) * wave_floats + r % p.wrows;
		dst[c * as] = v;
		float pw = 1.f;
		for (int j = 0; j < p.L; j++) {
			const double t = (double)(v * pw);   // an exact product
			dst[(p.D * (1 + 2 * j) + c) * as] = valid ? (float)sin(t) : 0.f;
			dst[(p.D * (2 + 2 * j) + c) * as] = valid ? (float)cos(t) : 0.f;
			pw = pw * 2.f;
		}
	}
}

template <int NT>
__device__ __forceinline__ void gsr_mlp_fill(gsr_f32x16 (&acc)[NT], const float* bias, int half)
{
#pragma unroll
	for (int t = 0; t < NT; t++) {
#pragma unroll
		for (int r = 0; r < 16; r++) acc[t][r] = bias ? bias[t * 32 + gsr_mlp_neuron(r, half)] : 0.f;
	}
}

// acc[t][i][row] = the chain fmaf(img[k][32 t + i], b[k][row], acc) over k = 0 .. 2 ksteps - 1 ascending.
// In a 16-row wave (as = 17) the lanes with col >= 16 read other rows' cells and, behind the last buffer, GSR_MLP_SLACK: whatever
// they read stays in their own column of the MFMA -- a column of D depends on that column of B alone -- and no such lane stores
// anything (wlane).  A reduction across lanes would break this; nothing here reduces across the columns of an accumulator.
template <int NT>
__device__ __forceinline__ void gsr_mlp_matmul(gsr_f32x16 (&acc)[NT], int ksteps, const float* img, const float* b, int as, int col, int half)
{
	constexpr int ST = gsr_mlp_stride(32 * NT);
	const float* ip = img + half * ST + col;
	const float* bp = b + half * as + col;
	for (int s = 0; s < ksteps; s++) {
		const float bv = bp[2 * s * as];
#pragma unroll
		for (int t = 0; t < NT; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ip[2 * s * ST + t * 32], bv, acc[t], 0, 0, 0);
	}
}

// z -> a into the wave's buffer a[k][row]; padded neurons and rows that do not exist are +0
template <int NT>
__device__ __forceinline__ void gsr_mlp_store_act(const gsr_f32x16 (&acc)[NT], int d, bool relu, bool valid, float* out, int as, int col, int half)
{
#pragma unroll
	for (int t = 0; t < NT; t++) {
#pragma unroll
		for (int r = 0; r < 16; r++) {
			const int o = t * 32 + gsr_mlp_neuron(r, half);
			float v = acc[t][r];
			if (relu) v = (v <= 0.f) ? 0.f : v;
			out[o * as + col] = (valid && o < d) ? v : 0.f;
		}
	}
}

__device__ __forceinline__ double gsr_mlp_sigmoid(double z) { return 1.0 / (1.0 + exp(-z)); }

// ---- forward ----
template <int NT>
__global__ void __launch_bounds__(512) gsr_mlp_forward_kernel(GsrMlpParams p)
{
	constexpr int P = 32 * NT, ST = gsr_mlp_stride(P);
	extern __shared__ __attribute__((aligned(16))) float lds[];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
	const int as = p.wrows + 1, rows = p.waves * p.wrows, wave_floats = P * as;
	float* img = lds;
	float* bias = lds + p.img_floats;
	float* bufs = bias + GSR_MLP_MAX_WIDTH;
	float* mine = bufs + wave * wave_floats;
	const long long row0 = (long long)blockIdx.x * rows;
	const bool valid = row0 + wave * p.wrows + col < p.N;

	gsr_mlp_load_input(p, row0, rows, bufs, wave_floats, as);
	gsr_f32x16 acc[NT];
	for (int l = 1; l <= p.M; l++) {
		const int din = p.d[l - 1], dout = p.d[l];
		gsr_sync();   // the image before has been read by every wave; the input is in place
		gsr_mlp_stage(img, p.prep + p.wt_off[l - 1], gsr_mlp_pad2(din) * ST);
		gsr_mlp_stage(bias, p.prep + p.bias_off[l - 1], P);
		gsr_sync();
		gsr_mlp_fill<NT>(acc, bias, half);
		gsr_mlp_matmul<NT>(acc, gsr_mlp_pad2(din) / 2, img, mine, as, col, half);
		// the last layer's z_M goes through the buffer as it is
		gsr_mlp_store_act<NT>(acc, dout, l < p.M && p.hidden == GSR_MLP_RELU, valid, mine, as, col, half);
	}
	// y = act(z_M), stored by the whole workgroup in the order of the output's layout
	const int dM = p.d[p.M];
	gsr_sync();
	for (int e = threadIdx.x; e < rows * dM; e += blockDim.x) {
		const int r = p.y_planes ? e % rows : e / dM, o = p.y_planes ? e / rows : e % dM;
		const long long row = row0 + r;
		if (row >= p.N) continue;
		float v = bufs[(r / p.wrows) * wave_floats + o * as + r % p.wrows];
		if (p.outact == GSR_MLP_SIGMOID) v = (float)gsr_mlp_sigmoid((double)v);
		if (p.outact == GSR_MLP_TANH) v = (float)tanh((double)v);
		if (p.y_planes) p.y[(size_t)o * p.ys + row] = v;
		else p.y[(size_t)row * p.ys + o] = v;
	}
}

// ---- backward ----
template <int NT>
__global__ void __launch_bounds__(256) gsr_mlp_backward_kernel(GsrMlpParams p)
{
	constexpr int P = 32 * NT, ST = gsr_mlp_stride(P);
	extern __shared__ __attribute__((aligned(16))) float lds[];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
	const int as = p.wrows + 1, rows = p.waves * p.wrows;
	const int wf = P * as, lf = p.waves * wf;   // floats of a wave's and of a layer's buffer
	float* img = lds;
	float* bias = lds + p.img_floats;
	float* acts = bias + GSR_MLP_MAX_WIDTH;   // a_0 .. a_{M-1}, a_l [waves][P][as] at l * lf
	float* dzb = acts + p.M * lf;             // dz_l [waves][P][as]
	float* dzmine = dzb + wave * wf;
	const bool wlane = col < p.wrows, relu = p.hidden == GSR_MLP_RELU;
	const int dM = p.d[p.M];
	float* part = p.part + (size_t)blockIdx.x * p.part_stride;

	for (int tile = blockIdx.x; tile < p.ntiles; tile += p.G) {
		const bool first = tile == (int)blockIdx.x;
		const long long row0 = (long long)tile * rows, row = row0 + wave * p.wrows + col;
		const bool valid = wlane && row < p.N;
		gsr_sync();   // the tile before has left the LDS
		gsr_mlp_load_input(p, row0, rows, acts, wf, as);
		gsr_f32x16 acc[NT];
		for (int l = 1; l <= p.M; l++) {
			const int din = p.d[l - 1], dout = p.d[l];
			gsr_sync();
			gsr_mlp_stage(img, p.prep + p.wt_off[l - 1], gsr_mlp_pad2(din) * ST);
			gsr_mlp_stage(bias, p.prep + p.bias_off[l - 1], P);
			gsr_sync();
			gsr_mlp_fill<NT>(acc, bias, half);
			gsr_mlp_matmul<NT>(acc, gsr_mlp_pad2(din) / 2, img, acts + (l - 1) * lf + wave * wf, as, col, half);
			// a_l beside the others; z_M, as it is, into the wave's part of dz's buffer
			if (wlane) gsr_mlp_store_act<NT>(acc, dout, l < p.M && relu, valid, l < p.M ? acts + l * lf + wave * wf : dzmine, as, col, half);
		}
		// each lane turns its own cells into dz_M = dy act'(z_M), a double product rounded once
		if (valid && p.outact != GSR_MLP_NONE) {
			for (int e = 0; e < NT * 16; e++) {
				const int o = (e >> 4) * 32 + gsr_mlp_neuron(e & 15, half);
				if (o >= dM) continue;
				const float g = p.y_planes ? p.dy[(size_t)o * p.dys + row] : p.dy[(size_t)row * p.dys + o];
				const double z = (double)dzmine[o * as + col];
				double da;
				if (p.outact == GSR_MLP_SIGMOID) da = gsr_mlp_sigmoid(z) * gsr_mlp_sigmoid(-z);
				else {
					const double th = tanh(z);
					da = 1.0 - th * th;
				}
				dzmine[o * as + col] = (float)((double)g * da);
			}
		} else if (valid) {
			for (int e = 0; e < NT * 16; e++) {
				const int o = (e >> 4) * 32 + gsr_mlp_neuron(e & 15, half);
				if (o < dM) dzmine[o * as + col] = p.y_planes ? p.dy[(size_t)o * p.dys + row] : p.dy[(size_t)row * p.dys + o];
			}
		}
		for (int l = p.M; l >= 1; l--) {
			const int din = p.d[l - 1], dout = p.d[l], ntk = (din + 31) / 32, nto = (dout + 31) / 32;
			const bool down = l > 1 || p.want_dx;
			const float* aprev = acts + (l - 1) * lf;   // a_{l-1}
			gsr_sync();   // dz_l is in place, the image free
			if (down) gsr_mlp_stage(img, p.prep + p.wb_off[l - 1], gsr_mlp_pad2(dout) * ST);
			if ((p.want_w >> (l - 1)) & 1) {
				// the 32 x 32 blocks of dW_l, one owner each: on top of the partial, the chain over the tile's rows in ascending order
				float* pw = part + p.pw_off[l - 1];
				for (int b = wave; b < nto * ntk; b += p.waves) {
					const int ot = b / ntk, kt = b % ntk, k = kt * 32 + col;
					gsr_f32x16 c;
#pragma unroll
					for (int r = 0; r < 16; r++) {
						const int o = ot * 32 + gsr_mlp_neuron(r, half);
						c[r] = (!first && o < dout && k < din) ? pw[(size_t)o * din + k] : 0.f;
					}
					for (int w2 = 0; w2 < p.waves; w2++) {
						const float* za = dzb + w2 * wf + (ot * 32 + col) * as + half;
						const float* ab = aprev + w2 * wf + (kt * 32 + col) * as + half;
						for (int s = 0; s < p.wrows / 2; s++) c = __builtin_amdgcn_mfma_f32_32x32x2f32(za[2 * s], ab[2 * s], c, 0, 0, 0);
					}
#pragma unroll
					for (int r = 0; r < 16; r++) {
						const int o = ot * 32 + gsr_mlp_neuron(r, half);
						if (o < dout && k < din) pw[(size_t)o * din + k] = c[r];
					}
				}
			}
			if ((p.want_b >> (l - 1)) & 1) {
				float* pb = part + p.pb_off[l - 1];
				for (int o = threadIdx.x; o < dout; o += blockDim.x) {
					float s = first ? 0.f : pb[o];
					for (int w2 = 0; w2 < p.waves; w2++)
						for (int r = 0; r < p.wrows; r++) s = s + dzb[w2 * wf + o * as + r];
					pb[o] = s;
				}
			}
			if (!down) break;
			gsr_sync();   // the image is staged
			gsr_mlp_fill<NT>(acc, nullptr, half);
			gsr_mlp_matmul<NT>(acc, gsr_mlp_pad2(dout) / 2, img, dzmine, as, col, half);
			gsr_sync();   // dz_l has been read by every wave
			if (wlane) {
				const float* am = aprev + wave * wf;
				const bool mask = l > 1 && relu;
#pragma unroll
				for (int t = 0; t < NT; t++) {
#pragma unroll
					for (int r = 0; r < 16; r++) {
						const int k = t * 32 + gsr_mlp_neuron(r, half);
						const bool keep = valid && k < din && (!mask || am[k * as + col] > 0.f);
						dzmine[k * as + col] = keep ? acc[t][r] : 0.f;
					}
				}
			}
		}
		if (p.want_dx) {
			// da_0 through the encoding, a lane per (row, raw column), in the order of x's layout
			gsr_sync();
			for (int e = threadIdx.x; e < rows * p.D; e += blockDim.x) {
				const int r = p.x_planes ? e % rows : e / p.D, c = p.x_planes ? e / rows : e % p.D;
				const long long xrow = row0 + r;
				if (xrow >= p.N) continue;
				const float* g = dzb + (r / p.wrows) * wf + r % p.wrows;
				float out = g[c * as];
				if (p.L > 0) {
					const float v = p.x_planes ? p.x[(size_t)c * p.xs + xrow] : p.x[(size_t)xrow * p.xs + c];
					double sum = (double)out;
					float pw = 1.f;
					for (int j = 0; j < p.L; j++) {
						const double t = (double)(v * pw);
						const double gs = (double)g[(p.D * (1 + 2 * j) + c) * as], gc = (double)g[(p.D * (2 + 2 * j) + c) * as];
						sum = sum + (double)pw * (cos(t) * gs - sin(t) * gc);
						pw = pw * 2.f;
					}
					out = (float)sum;
				}
				if (p.x_planes) p.dx[(size_t)c * p.dxs + xrow] = out;
				else p.dx[(size_t)xrow * p.dxs + c] = out;
			}
		}
	}
}

// dW_l and db_l = ((partial_0 + partial_1) + partial_2) .. in ascending workgroup order, one owner per element; blockIdx.y = layer - 1
__global__ void __launch_bounds__(256) gsr_mlp_fold_kernel(GsrMlpParams p, GsrMlpGrads g)
{
	const int l = blockIdx.y + 1, nw = p.d[l] * p.d[l - 1], nb = p.d[l];
	for (int e = blockIdx.x * 256 + threadIdx.x; e < nw + nb; e += gridDim.x * 256) {
		const bool w = e < nw;
		float* out = w ? g.dW[l - 1] : g.db[l - 1];
		if (!out) continue;
		const float* src = p.part + (w ? p.pw_off[l - 1] + e : p.pb_off[l - 1] + (e - nw));
		float s = src[0];
		for (int q = 1; q < p.G; q++) s = s + src[(size_t)q * p.part_stride];
		out[w ? e : e - nw] = s;
	}
}

// ---- host ----
struct GsrMlpPlan {
	int pmax, nt;                 // the widest padded layer, the instantiation's accumulators
	int img_floats;
	size_t prep_floats;
	int wt_off[GSR_MLP_MAX_LAYERS], wb_off[GSR_MLP_MAX_LAYERS], bias_off[GSR_MLP_MAX_LAYERS];
	int pw_off[GSR_MLP_MAX_LAYERS], pb_off[GSR_MLP_MAX_LAYERS];
	long long part_stride;
	int fwd_waves, fwd_wrows, bwd_waves, bwd_wrows;
	size_t fwd_lds, bwd_lds;
};

static bool gsr_mlp_shape_ok(const gsr_mlp_desc* d)
{
	if (!d || d->N < 0 || d->M < 1 || d->M > GSR_MLP_MAX_LAYERS || d->L < 0 || d->L > GSR_MLP_MAX_OCTAVES || d->D < 1) return false;
	for (int l = 0; l <= d->M; l++)
		if (d->widths[l] < 1 || d->widths[l] > GSR_MLP_MAX_WIDTH) return false;
	return (long long)d->D * (1 + 2 * d->L) == d->widths[0] && d->max_workgroups >= 0;
}

static size_t gsr_mlp_lds_bytes(const gsr_mlp_desc& d, const GsrMlpPlan& pl, int waves, int wrows, bool backward)
{
	size_t per_row_k = 0;   // k rows of the buffers of one wave
	per_row_k = (size_t)pl.pmax * (backward ? d.M + 1 : 1);
	return 4 * ((size_t)pl.img_floats + GSR_MLP_MAX_WIDTH + (size_t)waves * per_row_k * (wrows + 1) + GSR_MLP_SLACK);
}

static GsrMlpPlan gsr_mlp_plan(const gsr_mlp_desc& d)
{
	GsrMlpPlan pl = {};
	size_t off = 0;
	long long po = 0;
	for (int l = 0; l <= d.M; l++) pl.pmax = std::max(pl.pmax, gsr_mlp_pad32(d.widths[l]));
	pl.nt = pl.pmax / 32;
	for (int l = 1; l <= d.M; l++) {
		const int din = d.widths[l - 1], dout = d.widths[l];
		const int nt = gsr_mlp_pad2(din) * gsr_mlp_stride(pl.pmax), nb = gsr_mlp_pad2(dout) * gsr_mlp_stride(pl.pmax);
		pl.wt_off[l - 1] = (int)off; off += nt;
		pl.wb_off[l - 1] = (int)off; off += nb;
		pl.bias_off[l - 1] = (int)off; off += pl.pmax;
		pl.img_floats = std::max(pl.img_floats, std::max(nt, nb));
		pl.pw_off[l - 1] = (int)po; po += (long long)din * dout;
	}
	for (int l = 1; l <= d.M; l++) { pl.pb_off[l - 1] = (int)po; po += d.widths[l]; }
	pl.prep_floats = off;
	pl.part_stride = (po + 3) & ~3LL;
	pl.fwd_wrows = pl.bwd_wrows = 32;
	for (pl.fwd_waves = 8; pl.fwd_waves > 1 && gsr_mlp_lds_bytes(d, pl, pl.fwd_waves, 32, false) > GSR_MLP_LDS_BYTES; pl.fwd_waves /= 2) {}
	for (pl.bwd_waves = 4; pl.bwd_waves > 1 && gsr_mlp_lds_bytes(d, pl, pl.bwd_waves, 32, true) > GSR_MLP_LDS_BYTES; pl.bwd_waves /= 2) {}
	if (gsr_mlp_lds_bytes(d, pl, 1, 32, true) > GSR_MLP_LDS_BYTES) pl.bwd_wrows = 16;
	pl.fwd_lds = gsr_mlp_lds_bytes(d, pl, pl.fwd_waves, pl.fwd_wrows, false);
	pl.bwd_lds = gsr_mlp_lds_bytes(d, pl, pl.bwd_waves, pl.bwd_wrows, true);
	return pl;
}

static int gsr_mlp_groups(const gsr_mlp_desc& d, const GsrMlpPlan& pl, int* ntiles)
{
	const int R = pl.bwd_waves * pl.bwd_wrows;
	*ntiles = (int)(((long long)d.N + R - 1) / R);
	return std::min(*ntiles, d.max_workgroups ? d.max_workgroups : GSR_MLP_DEFAULT_WORKGROUPS);
}

extern "C" int gsr_mlp_tile_rows(const gsr_mlp_desc* desc)
{
	if (!gsr_mlp_shape_ok(desc)) return 0;
	const GsrMlpPlan pl = gsr_mlp_plan(*desc);
	return pl.bwd_waves * pl.bwd_wrows;
}

extern "C" size_t gsr_mlp_scratch_bytes(const gsr_mlp_desc* desc)
{
	if (!gsr_mlp_shape_ok(desc)) return 0;
	const GsrMlpPlan pl = gsr_mlp_plan(*desc);
	int ntiles;
	const int G = gsr_mlp_groups(*desc, pl, &ntiles);
	return gsr_align_up(4 * pl.prep_floats) + gsr_align_up(4 * (size_t)std::max(G, 1) * (size_t)pl.part_stride);
}

static int gsr_mlp_check(const char* who, const gsr_mlp_desc* d, const float* x, const float* const* weights, const void* out, const char* out_name,
                         const void* scratch, bool backward)
{
	if (!d) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: desc is NULL", who);
	if (d->N < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: negative count (N %d)", who, d->N);
	if (d->M < 1 || d->M > GSR_MLP_MAX_LAYERS) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: M must lie in 1..%d (got %d)", who, GSR_MLP_MAX_LAYERS, d->M);
	for (int l = 0; l <= d->M; l++)
		if (d->widths[l] < 1 || d->widths[l] > GSR_MLP_MAX_WIDTH)
			return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: widths[%d] must lie in 1..%d (got %d)", who, l, GSR_MLP_MAX_WIDTH, d->widths[l]);
	if (d->L < 0 || d->L > GSR_MLP_MAX_OCTAVES) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: L must lie in 0..%d (got %d)", who, GSR_MLP_MAX_OCTAVES, d->L);
	if (d->D < 1 || (long long)d->D * (1 + 2 * d->L) != d->widths[0])
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: widths[0] must be D (1 + 2 L) (D %d, L %d, widths[0] %d)", who, d->D, d->L, d->widths[0]);
	if (d->hidden_activation != GSR_MLP_NONE && d->hidden_activation != GSR_MLP_RELU)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: unknown hidden activation %d", who, d->hidden_activation);
	if (d->output_activation != GSR_MLP_NONE && d->output_activation != GSR_MLP_SIGMOID && d->output_activation != GSR_MLP_TANH)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: unknown output activation %d", who, d->output_activation);
	if ((d->x_layout != GSR_MLP_ROWS && d->x_layout != GSR_MLP_PLANES) || (d->y_layout != GSR_MLP_ROWS && d->y_layout != GSR_MLP_PLANES))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: unknown layout (x %d, y %d)", who, d->x_layout, d->y_layout);
	if (d->max_workgroups < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: negative max_workgroups (%d)", who, d->max_workgroups);
	const long long xmin = d->x_layout == GSR_MLP_PLANES ? d->N : d->D, ymin = d->y_layout == GSR_MLP_PLANES ? d->N : d->widths[d->M];
	if (d->x_stride < xmin || (!backward && d->y_stride < ymin) || (backward && d->dy_stride < ymin))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: a stride is smaller than its layout needs (x %lld of %lld, %s %lld of %lld)", who, d->x_stride, xmin,
		                backward ? "dy" : "y", backward ? d->dy_stride : d->y_stride, ymin);
	if (d->N == 0) return GSR_OK;
	if (!x || !weights || !out || !scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: x, weights, %s or scratch is NULL", who, out_name);
	for (int l = 0; l < d->M; l++)
		if (!weights[l]) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: weights[%d] is NULL", who, l);
	if ((uintptr_t)scratch & 15) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: scratch must be 16-byte aligned", who);
	return GSR_OK;
}

static GsrMlpParams gsr_mlp_params(const gsr_mlp_desc& d, const GsrMlpPlan& pl, const float* x, void* scratch)
{
	GsrMlpParams p = {};
	p.N = d.N; p.M = d.M; p.D = d.D; p.L = d.L;
	p.P = pl.pmax;
	p.hidden = d.hidden_activation; p.outact = d.output_activation;
	p.x_planes = d.x_layout == GSR_MLP_PLANES; p.y_planes = d.y_layout == GSR_MLP_PLANES;
	for (int l = 0; l <= d.M; l++) p.d[l] = d.widths[l];
	p.xs = d.x_stride; p.ys = d.y_stride; p.dys = d.dy_stride; p.dxs = d.dx_stride;
	p.x = x;
	p.prep = (const float*)scratch;
	for (int l = 0; l < d.M; l++) {
		p.wt_off[l] = pl.wt_off[l]; p.wb_off[l] = pl.wb_off[l]; p.bias_off[l] = pl.bias_off[l];
		p.pw_off[l] = pl.pw_off[l]; p.pb_off[l] = pl.pb_off[l];
	}
	p.img_floats = pl.img_floats;
	p.part = (float*)((char*)scratch + gsr_align_up(4 * pl.prep_floats));
	p.part_stride = pl.part_stride;
	return p;
}

static void gsr_mlp_prepare(const GsrMlpParams& p, const float* const* weights, const float* const* biases, hipStream_t s)
{
	GsrMlpWeights w = {};
	for (int l = 0; l < p.M; l++) {
		w.W[l] = weights[l];
		w.b[l] = biases ? biases[l] : nullptr;
	}
	hipLaunchKernelGGL(gsr_mlp_prepare_kernel, dim3(16, p.M), dim3(256), 0, s, p, w, (float*)p.prep);
}

// a kernel may take the whole LDS.  The limit above 64 KB belongs to the function on the current device, so it is raised on every
// call that needs it: no state, whichever device or host thread the call comes from
template <typename K>
static int gsr_mlp_raise_lds(K kernel, size_t lds)
{
	if (lds <= 64 * 1024) return GSR_OK;
	return gsr_check_hip(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, GSR_MLP_LDS_BYTES), "hipFuncSetAttribute(mlp)");
}

template <int NT>
static int gsr_mlp_launch_forward(const GsrMlpParams& p, size_t lds, hipStream_t s)
{
	if (const int rc = gsr_mlp_raise_lds(gsr_mlp_forward_kernel<NT>, lds)) return rc;
	const int rows = p.waves * p.wrows;
	hipLaunchKernelGGL(gsr_mlp_forward_kernel<NT>, dim3((unsigned)(((long long)p.N + rows - 1) / rows)), dim3(64 * p.waves), lds, s, p);
	return GSR_OK;
}

template <int NT>
static int gsr_mlp_launch_backward(const GsrMlpParams& p, size_t lds, hipStream_t s)
{
	if (const int rc = gsr_mlp_raise_lds(gsr_mlp_backward_kernel<NT>, lds)) return rc;
	hipLaunchKernelGGL(gsr_mlp_backward_kernel<NT>, dim3(p.G), dim3(64 * p.waves), lds, s, p);
	return GSR_OK;
}

extern "C" int gsr_mlp_forward(const gsr_mlp_desc* desc, const float* x, const float* const* weights, const float* const* biases, float* y, void* scratch,
                               void* stream)
{
	const char* who = "gsr_mlp_forward";
	if (const int rc = gsr_mlp_check(who, desc, x, weights, y, "y", scratch, false)) return rc;
	if (desc->N == 0) return GSR_OK;
	hipStream_t s = (hipStream_t)stream;
	GsrProfScope prof(s, "mlp_forward");
	const GsrMlpPlan pl = gsr_mlp_plan(*desc);
	GsrMlpParams p = gsr_mlp_params(*desc, pl, x, scratch);
	p.y = y;
	p.waves = pl.fwd_waves; p.wrows = pl.fwd_wrows;
	gsr_mlp_prepare(p, weights, biases, s);
	int rc;
	switch (pl.nt) {
	case 1: rc = gsr_mlp_launch_forward<1>(p, pl.fwd_lds, s); break;
	case 2: rc = gsr_mlp_launch_forward<2>(p, pl.fwd_lds, s); break;
	case 3: rc = gsr_mlp_launch_forward<3>(p, pl.fwd_lds, s); break;
	default: rc = gsr_mlp_launch_forward<4>(p, pl.fwd_lds, s); break;
	}
	if (rc) return rc;
	return gsr_stage_done(s, 0, "mlp_forward");
}

extern "C" int gsr_mlp_backward(const gsr_mlp_desc* desc, const float* x, const float* const* weights, const float* const* biases, const float* dy,
                                float* dx, float* const* dW, float* const* db, void* scratch, void* stream)
{
	const char* who = "gsr_mlp_backward";
	if (const int rc = gsr_mlp_check(who, desc, x, weights, dy, "dy", scratch, true)) return rc;
	hipStream_t s = (hipStream_t)stream;
	if (dx) {
		const long long need = desc->x_layout == GSR_MLP_PLANES ? desc->N : desc->D;
		if (desc->dx_stride < need)
			return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: a stride is smaller than its layout needs (dx %lld of %lld)", who, desc->dx_stride, need);
	}
	GsrMlpGrads g = {};
	unsigned want_w = 0, want_b = 0;
	for (int l = 0; l < desc->M; l++) {
		g.dW[l] = dW ? dW[l] : nullptr;
		g.db[l] = db ? db[l] : nullptr;
		want_w |= g.dW[l] ? 1u << l : 0u;
		want_b |= g.db[l] ? 1u << l : 0u;
	}
	if (desc->N == 0) {   // zeros to what is wanted
		for (int l = 0; l < desc->M; l++) {
			if (g.dW[l])
				if (const int rc = gsr_check_hip(hipMemsetAsync(g.dW[l], 0, 4 * (size_t)desc->widths[l] * desc->widths[l + 1], s), "hipMemsetAsync(dW)")) return rc;
			if (g.db[l])
				if (const int rc = gsr_check_hip(hipMemsetAsync(g.db[l], 0, 4 * (size_t)desc->widths[l + 1], s), "hipMemsetAsync(db)")) return rc;
		}
		return GSR_OK;
	}
	if (!dx && !want_w && !want_b) return GSR_OK;
	GsrProfScope prof(s, "mlp_backward");
	const GsrMlpPlan pl = gsr_mlp_plan(*desc);
	GsrMlpParams p = gsr_mlp_params(*desc, pl, x, scratch);
	p.dy = dy; p.dx = dx;
	p.want_dx = dx != nullptr; p.want_w = want_w; p.want_b = want_b;
	p.waves = pl.bwd_waves; p.wrows = pl.bwd_wrows;
	p.G = gsr_mlp_groups(*desc, pl, &p.ntiles);
	gsr_mlp_prepare(p, weights, biases, s);
	int rc;
	switch (pl.nt) {
	case 1: rc = gsr_mlp_launch_backward<1>(p, pl.bwd_lds, s); break;
	case 2: rc = gsr_mlp_launch_backward<2>(p, pl.bwd_lds, s); break;
	case 3: rc = gsr_mlp_launch_backward<3>(p, pl.bwd_lds, s); break;
	default: rc = gsr_mlp_launch_backward<4>(p, pl.bwd_lds, s); break;
	}
	if (rc) return rc;
	if (want_w || want_b) hipLaunchKernelGGL(gsr_mlp_fold_kernel, dim3(16, p.M), dim3(256), 0, s, p, g);
	return gsr_stage_done(s, 0, "mlp_backward");
}
