// hexplane.hip -- the HexPlane / K-Planes plane-grid encoding of include/gsr_hexplane.h: forward, the exact integer table gradient on
// its two paths, the row-owner dx, the plane regulariser.  The header writes the rule operation by operation; this unit is compiled
// uncontracted and the one fused operation of the rule (the per-plane chain) is written out.
//
// Launch shapes.
//   forward      one thread per (row, four channels): a corner is one 16-byte load, and the C / 4 lanes of a row read a node's 4 C
//                contiguous bytes and write 4 C contiguous bytes of y per level.
//   max          |dy|: grid-stride pass, wave maximum by shuffles, one integer atomicMax per wave on the sign-cleared bit pattern;
//                |table|: the same per plane.  prepare: one thread per plane turns the maxima into q (or "zero"), one flag says NaN.
//   direct       one thread per (row, channel), level slow: the lanes lie along the channels, so one no-return 64-bit integer
//                atomic instruction covers 64 / C nodes with 8 C contiguous bytes each -- whole lines, not one request per lane.
//   LDS          planes of at most 64 x 64 nodes: a workgroup owns one (plane, slice of four channels, row chunk), adds into LDS with
//                64-bit LDS atomics and flushes its non-zero sums once.  Adding an integer zero changes nothing, so skipping it
//                cannot change a bit.
//   convert      one thread per table element of the pass: sums -> dtable.
//   dx           one thread per row over every level, channel and plane: the gathers of the forward again, double accumulators.
//   regulariser  one thread per table element (grid-stride inside a plane's fixed number of workgroups), a tree per workgroup, a fold.
// Every node index is formed from i0 <= res - 2 and i0 + 1 inside its plane, every row index is checked against N.
#include "gsr_internal.h"
#include "gsr_depth_key.h"   // gsr_sync()
#include "../../include/gsr_hexplane.h"

#include <math.h>

#include <algorithm>

#define GSR_HP_LDS_GROUPS 64     // row chunks per (plane, slice) of the LDS path, at most
#define GSR_HP_LDS_THREADS 512
#define GSR_HP_WORDS_BYTES 512   // the small words in front of the sums
#define GSR_HP_W_M 0             // word 0: max |dy| bits; words 1 + flat plane: max |v| bits
#define GSR_HP_W_BAD 63          // != 0: a NaN or an infinity in dy or in table
#define GSR_HP_W_Q 64            // words 64 + flat plane: q as an int, or GSR_HP_Q_ZERO
#define GSR_HP_Q_ZERO (-0x7fffffff - 1)
#define GSR_HP_MAX_FLAT (GSR_HEXPLANE_MAX_LEVELS * GSR_HEXPLANE_MAX_PLANES)
#define GSR_HP_REG_BLOCKS 160    // workgroups per plane of the regulariser, at most: 48 x 160 partial sums of 8 bytes fit its scratch
#define GSR_HP_REG_ELEMENTS 2048 // elements per workgroup below which a plane takes fewer of them

struct GsrHpParams {
	int N, L, C, P, concat, B;
	long long xs, ys, dys, dxs;
	const float* x;
	const float* table;
	float* y;
	const float* dy;
	float* dx;
	float* dtable;
	unsigned long long* sums;   // the sums of the pass's planes, from pass_off on
	uint32_t* words;
	int pa, pb;                 // flat planes of the pass
	long long pass_off;
	int l0;                     // direct: first level of the launch
	int nent;                   // LDS: entries of the launch
	long long count;            // max: elements of dy
	int res[GSR_HEXPLANE_MAX_LEVELS][4];
	long long off[GSR_HP_MAX_FLAT + 1];
	unsigned char lds[GSR_HP_MAX_FLAT];   // the path per flat plane
	unsigned char ent[GSR_HP_MAX_FLAT];   // LDS: the flat planes of the launch
};

template <int V>
struct __attribute__((packed, aligned(4))) GsrHpVec {
	float v[V];
};

// the axes (a, b) of plane k
template <int D>
__host__ __device__ constexpr int gsr_hp_a(int k) { return D == 3 ? (k == 2 ? 1 : 0) : (k < 3 ? 0 : k < 5 ? 1 : 2); }
template <int D>
__host__ __device__ constexpr int gsr_hp_b(int k) { return D == 3 ? (k == 0 ? 1 : 2) : (k == 0 ? 1 : k == 1 ? 2 : k == 3 ? 2 : 3); }

// ---- the rule's per-row pieces ---------------------------------------------------------------------------------------------------
// -> false for a void row.  clamped: bit a set when u_a <= -1 or u_a >= 1
template <int D>
__device__ __forceinline__ bool gsr_hp_load_row(const float* __restrict__ xr, float u[D], unsigned* clamped)
{
	bool ok = true;
	unsigned cl = 0;
#pragma unroll
	for (int a = 0; a < D; a++) {
		const float v = xr[a];
		ok = ok && (fabsf(v) <= 3.402823466e38f);   // false for NaN and for +-inf
		cl |= (v <= -1.0f || v >= 1.0f) ? 1u << a : 0u;
		u[a] = v;
	}
	*clamped = cl;
	return ok;
}

// u finite
template <int D>
__device__ __forceinline__ void gsr_hp_position(const float u[D], const int* __restrict__ res, int i0[D], float frac[D])
{
#pragma unroll
	for (int a = 0; a < D; a++) {
		const int r = res[a];
		const double top = (double)(r - 1);
		const double t0 = (double)u[a] + 1.0;
		const double t1 = t0 * 0.5;
		double s = t1 * top;
		s = s < 0.0 ? 0.0 : s > top ? top : s;
		const int i = min((int)floor(s), r - 2);
		i0[a] = i;
		frac[a] = (float)(s - (double)i);
	}
}

// the four corner values of V channels from c0 on, in the corner order
template <int V>
__device__ __forceinline__ void gsr_hp_corners(const float* __restrict__ plane, uint32_t node, int ra, int C, int c0, GsrHpVec<V> v[4])
{
	const uint32_t e = node * (uint32_t)C + (uint32_t)c0, rowb = (uint32_t)ra * (uint32_t)C;   // < 2^30 + 2^19
	v[0] = *(const GsrHpVec<V>*)(plane + e);
	v[1] = *(const GsrHpVec<V>*)(plane + e + C);
	v[2] = *(const GsrHpVec<V>*)(plane + e + rowb);
	v[3] = *(const GsrHpVec<V>*)(plane + e + rowb + C);
}

__device__ __forceinline__ void gsr_hp_weights(float fa, float fb, float w[4])
{
	const float a0 = 1.0f - fa, b0 = 1.0f - fb;
	w[0] = b0 * a0;
	w[1] = b0 * fa;
	w[2] = fb * a0;
	w[3] = fb * fa;
}

template <int V>
__device__ __forceinline__ void gsr_hp_chain(const float w[4], const GsrHpVec<V> v[4], float p[V])
{
#pragma unroll
	for (int i = 0; i < V; i++) {
		float acc = 0.0f;
#pragma unroll
		for (int k = 0; k < 4; k++) acc = __builtin_fmaf(w[k], v[k].v[i], acc);
		p[i] = acc;
	}
}

// p[k][0 .. V) of every plane of level l for the channels from c0 on; node[k] = ib * res_a + ia of the first corner
template <int D, int V>
__device__ __forceinline__ void gsr_hp_planes(const GsrHpParams& p, int l, const int i0[D], const float frac[D], int c0, float out[D * (D - 1) / 2][V],
                                              uint32_t node[D * (D - 1) / 2])
{
#pragma unroll
	for (int k = 0; k < D * (D - 1) / 2; k++) {
		const int a = gsr_hp_a<D>(k), b = gsr_hp_b<D>(k);
		const int ra = p.res[l][a];
		node[k] = (uint32_t)i0[b] * (uint32_t)ra + (uint32_t)i0[a];
		GsrHpVec<V> v[4];
		gsr_hp_corners<V>(p.table + p.off[l * p.P + k], node[k], ra, p.C, c0, v);
		float w[4];
		gsr_hp_weights(frac[a], frac[b], w);
		gsr_hp_chain<V>(w, v, out[k]);
	}
}

__device__ __forceinline__ double gsr_hp_pow2(int q)   // 2^q as a double, q in -1022 .. 1023: multiplying by it is ldexp
{
	return __longlong_as_double((long long)(q + 1023) << 52);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(256) gsr_hp_forward_kernel(GsrHpParams p)
{
	constexpr int P = D * (D - 1) / 2;
	const int CQ = p.C >> 2;
	const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
	const long long i = t / CQ;
	if (i >= p.N) return;
	const int c0 = (int)(t - i * CQ) * 4;
	float u[D];
	unsigned clamped;
	const bool ok = gsr_hp_load_row<D>(p.x + i * p.xs, u, &clamped);
	GsrHpVec<4> sum;
#pragma unroll
	for (int c = 0; c < 4; c++) sum.v[c] = 0.0f;
	for (int l = 0; l < p.L; l++) {
		GsrHpVec<4> z;
#pragma unroll
		for (int c = 0; c < 4; c++) z.v[c] = 0.0f;
		if (ok) {
			int i0[D];
			float frac[D];
			gsr_hp_position<D>(u, p.res[l], i0, frac);
			float pk[P][4];
			uint32_t node[P];
			gsr_hp_planes<D, 4>(p, l, i0, frac, c0, pk, node);
#pragma unroll
			for (int c = 0; c < 4; c++) {
				float v = pk[0][c];
#pragma unroll
				for (int k = 1; k < P; k++) v = v * pk[k][c];
				z.v[c] = v;
			}
		}
		if (p.concat) *(GsrHpVec<4>*)(p.y + i * p.ys + (long long)l * p.C + c0) = z;
		else {
#pragma unroll
			for (int c = 0; c < 4; c++) sum.v[c] = sum.v[c] + z.v[c];
		}
	}
	if (!p.concat) *(GsrHpVec<4>*)(p.y + i * p.ys + c0) = sum;
}

// ---- the maxima and q ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void gsr_hp_wave_max(uint32_t m, uint32_t* word)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
	if ((threadIdx.x & 63) == 0 && m) atomicMax(word, m);
}

__global__ void __launch_bounds__(256) gsr_hp_max_dy_kernel(GsrHpParams p, int cols)
{
	uint32_t m = 0;
	for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < p.count; j += (long long)gridDim.x * 256) {
		const long long row = j / cols;
		const int col = (int)(j - row * cols);
		m = max(m, __float_as_uint(p.dy[row * p.dys + col]) & 0x7fffffffu);
	}
	gsr_hp_wave_max(m, p.words + GSR_HP_W_M);
}

__global__ void __launch_bounds__(256) gsr_hp_max_table_kernel(GsrHpParams p)
{
	const int fp = (int)blockIdx.y;
	const float* __restrict__ plane = p.table + p.off[fp];
	const long long n = p.off[fp + 1] - p.off[fp];
	uint32_t m = 0;
	for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256)
		m = max(m, __float_as_uint(plane[j]) & 0x7fffffffu);
	gsr_hp_wave_max(m, p.words + 1 + fp);
}

// one workgroup of 64 threads: thread fp forms q of its plane
__global__ void __launch_bounds__(64) gsr_hp_prepare_kernel(GsrHpParams p)
{
	const int fp = (int)threadIdx.x, LP = p.L * p.P;
	if (fp == 0) {
		uint32_t bad = 0;
		for (int j = 0; j <= LP; j++) bad |= p.words[j] >= 0x7f800000u;
		p.words[GSR_HP_W_BAD] = bad;
	}
	if (fp >= LP) return;
	const int l = fp / p.P, k = fp - l * p.P;
	double bnd = (double)__uint_as_float(p.words[GSR_HP_W_M]);
	for (int j = 0; j < p.P; j++)
		if (j != k) bnd = bnd * (double)__uint_as_float(p.words[1 + l * p.P + j]);
	int q = GSR_HP_Q_ZERO;
	if (bnd > 0.0) {   // false for 0 and for a NaN (which the flag covers)
		const int e = (int)((__double_as_longlong(bnd) >> 52) & 0x7ff) - 1023 + 2;   // bnd >= 2^-894 is a normal double
		q = 62 - p.B - e;
	}
	((int*)p.words)[GSR_HP_W_Q + fp] = q;
}

// ---- the table gradient ----------------------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(256) gsr_hp_grad_direct_kernel(GsrHpParams p)
{
	constexpr int P = D * (D - 1) / 2;
	if (p.words[GSR_HP_W_BAD]) return;
	const int l = p.l0 + (int)blockIdx.y;
	bool any = false;   // uniform: a level of the pass whose planes all take the LDS path has nothing to do here
#pragma unroll
	for (int k = 0; k < P; k++) any = any || (!p.lds[l * P + k] && l * P + k >= p.pa && l * P + k < p.pb);
	if (!any) return;
	const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
	const long long i = t / p.C;
	if (i >= p.N) return;
	const int c = (int)(t - i * p.C);
	float u[D];
	unsigned clamped;
	if (!gsr_hp_load_row<D>(p.x + i * p.xs, u, &clamped)) return;
	int i0[D];
	float frac[D];
	gsr_hp_position<D>(u, p.res[l], i0, frac);
	float pk[P][1];
	uint32_t node[P];
	gsr_hp_planes<D, 1>(p, l, i0, frac, c, pk, node);
	const double g0 = (double)p.dy[i * p.dys + (p.concat ? (long long)l * p.C : 0) + c];
#pragma unroll
	for (int k = 0; k < P; k++) {
		const int fp = l * P + k;
		if (p.lds[fp] || fp < p.pa || fp >= p.pb) continue;
		const int q = ((const int*)p.words)[GSR_HP_W_Q + fp];
		if (q == GSR_HP_Q_ZERO) continue;
		double g = g0;
#pragma unroll
		for (int j = 0; j < P; j++)
			if (j != k) g = g * (double)pk[j][0];
		const double pow2q = gsr_hp_pow2(q);
		const int a = gsr_hp_a<D>(k), b = gsr_hp_b<D>(k);
		float w[4];
		gsr_hp_weights(frac[a], frac[b], w);
		const uint32_t C = (uint32_t)p.C, rowb = (uint32_t)p.res[l][a] * C;
		unsigned long long* __restrict__ s = p.sums + (p.off[fp] - p.pass_off) + (node[k] * C + (uint32_t)c);
		const uint32_t at[4] = {0, C, rowb, rowb + C};
#pragma unroll
		for (int n = 0; n < 4; n++) {
			const double prod = (double)w[n] * g;
			const long long v = __double2ll_rn(prod * pow2q);
			if (v) (void)__hip_atomic_fetch_add(s + at[n], (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	}
}

template <int D>
__global__ void __launch_bounds__(GSR_HP_LDS_THREADS) gsr_hp_grad_lds_kernel(GsrHpParams p)
{
	constexpr int P = D * (D - 1) / 2;
	extern __shared__ unsigned long long gsr_hp_lds[];
	if (p.words[GSR_HP_W_BAD]) return;   // uniform: in front of every barrier
	const int fp = p.ent[blockIdx.z];
	const int q = ((const int*)p.words)[GSR_HP_W_Q + fp];
	if (q == GSR_HP_Q_ZERO) return;      // uniform
	const int l = fp / P, k = fp - l * P;
	const int c0 = (int)blockIdx.y * 4;
	int ra = 0, rb = 0;
#pragma unroll
	for (int kk = 0; kk < P; kk++)
		if (kk == k) { ra = p.res[l][gsr_hp_a<D>(kk)]; rb = p.res[l][gsr_hp_b<D>(kk)]; }
	const uint32_t n = (uint32_t)(ra * rb) * 4;   // <= GSR_HEXPLANE_LDS_BYTES / 8 by the path's rule
	for (uint32_t j = threadIdx.x; j < n; j += GSR_HP_LDS_THREADS) gsr_hp_lds[j] = 0;
	gsr_sync();
	const double pow2q = gsr_hp_pow2(q);
	for (long long tile = blockIdx.x; tile * GSR_HP_LDS_THREADS < p.N; tile += gridDim.x) {
		const long long i = tile * GSR_HP_LDS_THREADS + threadIdx.x;
		if (i >= p.N) continue;
		float u[D];
		unsigned clamped;
		if (!gsr_hp_load_row<D>(p.x + i * p.xs, u, &clamped)) continue;
		int i0[D];
		float frac[D];
		gsr_hp_position<D>(u, p.res[l], i0, frac);
		float pk[P][4];
		uint32_t node[P];
		gsr_hp_planes<D, 4>(p, l, i0, frac, c0, pk, node);
		uint32_t nd = 0;
		float fa = 0.0f, fb = 0.0f;
#pragma unroll
		for (int kk = 0; kk < P; kk++)
			if (kk == k) { nd = node[kk]; fa = frac[gsr_hp_a<D>(kk)]; fb = frac[gsr_hp_b<D>(kk)]; }
		float w[4];
		gsr_hp_weights(fa, fb, w);
		const GsrHpVec<4> dyv = *(const GsrHpVec<4>*)(p.dy + i * p.dys + (p.concat ? (long long)l * p.C : 0) + c0);
		const uint32_t at[4] = {nd * 4, (nd + 1) * 4, (nd + (uint32_t)ra) * 4, (nd + (uint32_t)ra + 1) * 4};   // < n: nd + ra + 1 <= ra rb - 1
#pragma unroll
		for (int c = 0; c < 4; c++) {
			double g = (double)dyv.v[c];
#pragma unroll
			for (int j = 0; j < P; j++)
				if (j != k) g = g * (double)pk[j][c];
#pragma unroll
			for (int m = 0; m < 4; m++) {
				const double prod = (double)w[m] * g;
				const long long v = __double2ll_rn(prod * pow2q);
				if (v) (void)__hip_atomic_fetch_add(gsr_hp_lds + at[m] + c, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			}
		}
	}
	gsr_sync();
	unsigned long long* __restrict__ sums = p.sums + (p.off[fp] - p.pass_off) + c0;
	for (uint32_t j = threadIdx.x; j < n; j += GSR_HP_LDS_THREADS) {
		const unsigned long long v = gsr_hp_lds[j];
		if (v) (void)__hip_atomic_fetch_add(sums + (size_t)(j >> 2) * p.C + (j & 3), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// sums of the pass -> dtable; blockIdx.y: the plane within the pass
__global__ void __launch_bounds__(256) gsr_hp_convert_kernel(GsrHpParams p)
{
	const int fp = p.pa + (int)blockIdx.y;
	const long long n = p.off[fp + 1] - p.off[fp];
	const uint32_t bad = p.words[GSR_HP_W_BAD];
	const int q = ((const int*)p.words)[GSR_HP_W_Q + fp];
	const unsigned long long* __restrict__ s = p.sums + (p.off[fp] - p.pass_off);
	float* __restrict__ out = p.dtable + p.off[fp];
	const double scale = (bad || q == GSR_HP_Q_ZERO) ? 0.0 : gsr_hp_pow2(-q);
	for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256) {
		float v = 0.0f;
		if (bad) v = __uint_as_float(0x7fc00000u);
		else if (q != GSR_HP_Q_ZERO) v = (float)((double)(long long)s[j] * scale);
		out[j] = v;
	}
}

// ---- dx --------------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(256) gsr_hp_dx_kernel(GsrHpParams p)
{
	constexpr int P = D * (D - 1) / 2;
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i >= p.N) return;
	float u[D];
	unsigned clamped;
	const bool ok = gsr_hp_load_row<D>(p.x + i * p.xs, u, &clamped);
	double acc[D];
#pragma unroll
	for (int a = 0; a < D; a++) acc[a] = 0.0;
	if (ok) {
		for (int l = 0; l < p.L; l++) {
			int i0[D];
			float frac[D];
			gsr_hp_position<D>(u, p.res[l], i0, frac);
			double half[D];
#pragma unroll
			for (int a = 0; a < D; a++) half[a] = (double)(p.res[l][a] - 1) * 0.5;
			const float* __restrict__ dyl = p.dy + i * p.dys + (p.concat ? (long long)l * p.C : 0);
			for (int c0 = 0; c0 < p.C; c0 += 4) {
				float pk[P][4];
				double da[P][4], db[P][4];
#pragma unroll
				for (int k = 0; k < P; k++) {
					const int a = gsr_hp_a<D>(k), b = gsr_hp_b<D>(k);
					const int ra = p.res[l][a];
					GsrHpVec<4> v[4];
					gsr_hp_corners<4>(p.table + p.off[l * P + k], (uint32_t)i0[b] * (uint32_t)ra + (uint32_t)i0[a], ra, p.C, c0, v);
					float w[4];
					gsr_hp_weights(frac[a], frac[b], w);
					gsr_hp_chain<4>(w, v, pk[k]);
					const double fa = (double)frac[a], fb = (double)frac[b], a0 = (double)(1.0f - frac[a]), b0 = (double)(1.0f - frac[b]);
#pragma unroll
					for (int c = 0; c < 4; c++) {
						const double v00 = (double)v[0].v[c], v01 = (double)v[1].v[c], v10 = (double)v[2].v[c], v11 = (double)v[3].v[c];
						da[k][c] = b0 * (v01 - v00) + fb * (v11 - v10);
						db[k][c] = a0 * (v10 - v00) + fa * (v11 - v01);
					}
				}
				const GsrHpVec<4> g4 = *(const GsrHpVec<4>*)(dyl + c0);
#pragma unroll
				for (int c = 0; c < 4; c++) {
#pragma unroll
					for (int k = 0; k < P; k++) {
						double g = (double)g4.v[c];
#pragma unroll
						for (int j = 0; j < P; j++)
							if (j != k) g = g * (double)pk[j][c];
						acc[gsr_hp_a<D>(k)] += g * half[gsr_hp_a<D>(k)] * da[k][c];
						acc[gsr_hp_b<D>(k)] += g * half[gsr_hp_b<D>(k)] * db[k][c];
					}
				}
			}
		}
	}
#pragma unroll
	for (int a = 0; a < D; a++) p.dx[i * p.dxs + a] = (ok && !(clamped >> a & 1)) ? (float)acc[a] : 0.0f;
}

// ---- regulariser -----------------------------------------------------------------------------------------------------------------
struct GsrHpReg {
	double tv[2], smooth[2], l1;   // [0] space, [1] time
};

__device__ __forceinline__ double gsr_hp_block_sum(double v, double* sh)
{
	sh[threadIdx.x] = v;
	gsr_sync();
	for (int d = 128; d >= 1; d >>= 1) {
		if ((int)threadIdx.x < d) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + d];
		gsr_sync();
	}
	return sh[0];
}

// workgroups of a plane of n elements: a function of the shape alone, so the order of the sums is one
__host__ __device__ inline int gsr_hp_reg_blocks(long long n)
{
	const long long b = (n + GSR_HP_REG_ELEMENTS - 1) / GSR_HP_REG_ELEMENTS;
	return (int)(b < 1 ? 1 : b > GSR_HP_REG_BLOCKS ? GSR_HP_REG_BLOCKS : b);
}

// grid (GSR_HP_REG_BLOCKS, L P): partial[fp * GSR_HP_REG_BLOCKS + blockIdx.x], 0 from the workgroups a small plane does not use
__global__ void __launch_bounds__(256) gsr_hp_reg_kernel(GsrHpParams p, GsrHpReg w, int D, double* __restrict__ partial)
{
	__shared__ double sh[256];
	const int fp = (int)blockIdx.y;
	const int l = fp / p.P, k = fp - l * p.P;
	const int a = D == 3 ? gsr_hp_a<3>(k) : gsr_hp_a<4>(k), b = D == 3 ? gsr_hp_b<3>(k) : gsr_hp_b<4>(k);
	const int tp = b == 3;   // a time plane
	const long long ra = p.res[l][a], rb = p.res[l][b], C = p.C;
	const long long sa = C, sb = ra * C, n = rb * sb;
	const float* __restrict__ v = p.table + p.off[fp];
	const double kb = 2.0 * w.tv[tp] / (double)((rb - 1) * ra * C), ka = 2.0 * w.tv[tp] / (double)(rb * (ra - 1) * C);
	const double ks = rb >= 3 ? w.smooth[tp] / (double)((rb - 2) * ra * C) : 0.0;
	const double kl = tp ? w.l1 / (double)n : 0.0;
	const int nb = gsr_hp_reg_blocks(n);
	if ((int)blockIdx.x >= nb) {   // uniform
		if (threadIdx.x == 0) partial[fp * GSR_HP_REG_BLOCKS + blockIdx.x] = 0.0;
		return;
	}
	double val = 0.0;
	for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)nb * 256) {
		const long long ib = j / sb, ia = (j - ib * sb) / C;
		const double x = (double)v[j];
		double g = 0.0;
		// first differences: the term of (j, j + stride) is owned by j
		if (ib + 1 < rb) { const double d = (double)v[j + sb] - x; val += kb * d * d; g -= 2.0 * kb * d; }
		if (ib > 0) g += 2.0 * kb * (x - (double)v[j - sb]);
		if (ia + 1 < ra) { const double d = (double)v[j + sa] - x; val += ka * d * d; g -= 2.0 * ka * d; }
		if (ia > 0) g += 2.0 * ka * (x - (double)v[j - sa]);
		// second differences along b: s_i = v[i + 2] - 2 v[i + 1] + v[i], owned by i
		if (ks != 0.0) {
			if (ib + 2 < rb) { const double s = ((double)v[j + 2 * sb] - 2.0 * (double)v[j + sb]) + x; val += ks * s * s; g += 2.0 * ks * s; }
			if (ib >= 1 && ib + 1 < rb) { const double s = ((double)v[j + sb] - 2.0 * x) + (double)v[j - sb]; g -= 4.0 * ks * s; }
			if (ib >= 2) { const double s = (x - 2.0 * (double)v[j - sb]) + (double)v[j - 2 * sb]; g += 2.0 * ks * s; }
		}
		if (kl != 0.0) {
			const double d = 1.0 - x;
			val += kl * fabs(d);
			g += d > 0.0 ? -kl : d < 0.0 ? kl : 0.0;
		}
		if (p.dtable) p.dtable[p.off[fp] + j] = (float)g;
	}
	const double s = gsr_hp_block_sum(val, sh);
	if (threadIdx.x == 0) partial[fp * GSR_HP_REG_BLOCKS + blockIdx.x] = s;
}

__global__ void __launch_bounds__(256) gsr_hp_reg_fold_kernel(const double* __restrict__ partial, int n, float* __restrict__ value)
{
	__shared__ double sh[256];
	double v = 0.0;
	for (int j = threadIdx.x; j < n; j += 256) v += partial[j];
	const double s = gsr_hp_block_sum(v, sh);
	if (threadIdx.x == 0) *value = (float)s;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// NULL when the desc's shape lies inside the limits (N and the strides aside), else what is wrong with it
static const char* gsr_hp_shape_error(const gsr_hexplane_desc* d)
{
	if (!d) return "desc is NULL";
	if (d->D != 3 && d->D != 4) return "D must be 3 or 4";
	if (d->L < 1 || d->L > GSR_HEXPLANE_MAX_LEVELS) return "L must lie in 1..8";
	if (d->C < 4 || d->C > 64 || d->C % 4) return "C must be a multiple of 4 in 4..64";
	for (int l = 0; l < d->L; l++)
		for (int a = 0; a < d->D; a++)
			if (d->res[l][a] < 2 || d->res[l][a] > GSR_HEXPLANE_MAX_RES) return "a resolution must lie in 2..4096";
	return nullptr;
}

static void gsr_hp_axes(int D, int k, int* a, int* b)
{
	*a = D == 3 ? gsr_hp_a<3>(k) : gsr_hp_a<4>(k);
	*b = D == 3 ? gsr_hp_b<3>(k) : gsr_hp_b<4>(k);
}

static long long gsr_hp_nodes(const gsr_hexplane_desc& d, int l, int k)
{
	int a, b;
	gsr_hp_axes(d.D, k, &a, &b);
	return (long long)d.res[l][a] * d.res[l][b];
}

static bool gsr_hp_lds_plane(const gsr_hexplane_desc& d, int l, int k)
{
	return (size_t)gsr_hp_nodes(d, l, k) * 4 * 8 <= GSR_HEXPLANE_LDS_BYTES;
}

// the offsets and paths of a desc that passed gsr_hp_shape_error
static GsrHpParams gsr_hp_params(const gsr_hexplane_desc& d)
{
	GsrHpParams p = {};
	p.N = d.N; p.L = d.L; p.C = d.C; p.P = d.D * (d.D - 1) / 2; p.concat = d.concat != 0;
	p.xs = d.x_stride; p.ys = d.y_stride; p.dys = d.dy_stride; p.dxs = d.dx_stride;
	long long off = 0;
	for (int l = 0; l < d.L; l++) {
		for (int a = 0; a < d.D; a++) p.res[l][a] = d.res[l][a];
		for (int k = 0; k < p.P; k++) {
			p.off[l * p.P + k] = off;
			p.lds[l * p.P + k] = gsr_hp_lds_plane(d, l, k);
			off += gsr_hp_nodes(d, l, k) * d.C;
		}
	}
	p.off[d.L * p.P] = off;
	return p;
}

extern "C" int gsr_hexplane_layout(const gsr_hexplane_desc* desc, long long* offsets)
{
	if (const char* e = gsr_hp_shape_error(desc)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_hexplane_layout: %s", e);
	if (!offsets) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_hexplane_layout: offsets is NULL");
	const GsrHpParams p = gsr_hp_params(*desc);
	for (int j = 0; j <= p.L * p.P; j++) offsets[j] = p.off[j];
	return GSR_OK;
}

extern "C" int gsr_hexplane_level_path(const gsr_hexplane_desc* desc, int level, int plane)
{
	if (gsr_hp_shape_error(desc) || level < 0 || level >= desc->L || plane < 0 || plane >= desc->D * (desc->D - 1) / 2) return -1;
	return gsr_hp_lds_plane(*desc, level, plane) ? GSR_HEXPLANE_PATH_LDS : GSR_HEXPLANE_PATH_DIRECT;
}

static void gsr_hp_scratch(const GsrHpParams& p, size_t* min_bytes, size_t* full_bytes)
{
	long long largest = 0;
	for (int j = 0; j < p.L * p.P; j++) largest = std::max(largest, p.off[j + 1] - p.off[j]);
	if (min_bytes) *min_bytes = GSR_HP_WORDS_BYTES + (size_t)largest * 8;
	if (full_bytes) *full_bytes = GSR_HP_WORDS_BYTES + (size_t)p.off[p.L * p.P] * 8;
}

extern "C" int gsr_hexplane_scratch_bytes(const gsr_hexplane_desc* desc, size_t* min_bytes, size_t* full_bytes)
{
	if (min_bytes) *min_bytes = 0;
	if (full_bytes) *full_bytes = 0;
	if (const char* e = gsr_hp_shape_error(desc)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_hexplane_scratch_bytes: %s", e);
	gsr_hp_scratch(gsr_hp_params(*desc), min_bytes, full_bytes);
	return GSR_OK;
}

static int gsr_hp_check(const char* who, const gsr_hexplane_desc* d, const float* x, const float* table, const void* io, const char* io_name, bool backward)
{
	if (const char* e = gsr_hp_shape_error(d)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: %s", who, e);
	if (d->N < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: negative count (N %d)", who, d->N);
	const long long cols = d->concat ? (long long)d->L * d->C : d->C;
	if (d->x_stride < d->D || (!backward && d->y_stride < cols) || (backward && d->dy_stride < cols))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: a stride is smaller than its column count (x %lld of %d, %s %lld of %lld)", who, d->x_stride, d->D,
		                backward ? "dy" : "y", backward ? d->dy_stride : d->y_stride, cols);
	if (d->N == 0) return GSR_OK;
	if (!x || !table || !io) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: x, table or %s is NULL", who, io_name);
	return GSR_OK;
}

static int gsr_hp_check_scratch(const char* who, const void* scratch, size_t scratch_bytes, size_t min_bytes)
{
	if (!scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: scratch is NULL", who);
	if ((uintptr_t)scratch & 15) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: scratch must be 16-byte aligned", who);
	if (scratch_bytes < min_bytes)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: scratch is below the minimum (%zu of %zu bytes)", who, scratch_bytes, min_bytes);
	return GSR_OK;
}

// f(D as an integral constant) for the desc's D
template <typename Fn>
static inline void gsr_hp_variant(int D, Fn&& f)
{
	if (D == 3) f(std::integral_constant<int, 3>{});
	else f(std::integral_constant<int, 4>{});
}

static unsigned gsr_hp_blocks(long long n, long long cap)
{
	return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, cap));
}

extern "C" int gsr_hexplane_forward(const gsr_hexplane_desc* desc, const float* x, const float* table, float* y, void* stream)
{
	const char* who = "gsr_hexplane_forward";
	if (const int rc = gsr_hp_check(who, desc, x, table, y, "y", false)) return rc;
	if (desc->N == 0) return GSR_OK;
	hipStream_t s = (hipStream_t)stream;
	GsrProfScope prof(s, "hexplane_forward");
	GsrHpParams p = gsr_hp_params(*desc);
	p.x = x; p.table = table; p.y = y;
	const long long threads = (long long)desc->N * (desc->C / 4);   // < 2^35: the grid fits
	gsr_hp_variant(desc->D, [&](auto DD) {
		hipLaunchKernelGGL((gsr_hp_forward_kernel<DD()>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, p);
	});
	return gsr_stage_done(s, 0, "hexplane_forward");
}

extern "C" int gsr_hexplane_backward(const gsr_hexplane_desc* desc, const float* x, const float* table, const float* dy, float* dx, float* dtable,
                                     void* scratch, size_t scratch_bytes, void* stream)
{
	const char* who = "gsr_hexplane_backward";
	if (const int rc = gsr_hp_check(who, desc, x, table, dy, "dy", true)) return rc;
	if (dx && desc->dx_stride < desc->D)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: a stride is smaller than its column count (dx %lld of %d)", who, desc->dx_stride, desc->D);
	hipStream_t s = (hipStream_t)stream;
	GsrHpParams p = gsr_hp_params(*desc);
	const int LP = p.L * p.P, C = desc->C;
	const long long total = p.off[LP];
	if (desc->N == 0) {
		if (dtable) return gsr_check_hip(hipMemsetAsync(dtable, 0, (size_t)total * 4, s), "hipMemsetAsync(dtable)");
		return GSR_OK;
	}
	if (dtable) {
		size_t min_bytes = 0;
		gsr_hp_scratch(p, &min_bytes, nullptr);
		if (const int rc = gsr_hp_check_scratch(who, scratch, scratch_bytes, min_bytes)) return rc;
	}
	if (!dx && !dtable) return GSR_OK;
	GsrProfScope prof(s, "hexplane_backward");
	p.x = x; p.table = table; p.dy = dy; p.dx = dx; p.dtable = dtable;
	if (dx)
		gsr_hp_variant(desc->D, [&](auto DD) {
			hipLaunchKernelGGL((gsr_hp_dx_kernel<DD()>), dim3((unsigned)(((long long)desc->N + 255) / 256)), dim3(256), 0, s, p);
		});
	if (dtable) {
		p.words = (uint32_t*)scratch;
		p.sums = (unsigned long long*)((char*)scratch + GSR_HP_WORDS_BYTES);
		for (p.B = 0; (1ull << p.B) < 4ull * (unsigned long long)desc->N; p.B++) {}
		if (const int rc = gsr_check_hip(hipMemsetAsync(p.words, 0, GSR_HP_WORDS_BYTES, s), "hipMemsetAsync(hexplane words)")) return rc;
		const int cols = desc->concat ? desc->L * C : C;
		p.count = (long long)desc->N * cols;
		hipLaunchKernelGGL(gsr_hp_max_dy_kernel, dim3(gsr_hp_blocks(p.count, 2048)), dim3(256), 0, s, p, cols);
		hipLaunchKernelGGL(gsr_hp_max_table_kernel, dim3(gsr_hp_blocks(total / LP, 256), LP), dim3(256), 0, s, p);
		hipLaunchKernelGGL(gsr_hp_prepare_kernel, dim3(1), dim3(64), 0, s, p);
		const size_t capacity = (scratch_bytes - GSR_HP_WORDS_BYTES) / 8;   // elements whose sums the scratch holds
		const long long row_blocks = ((long long)desc->N * C + 255) / 256;   // < 2^29
		for (int pa = 0; pa < LP;) {
			int pb = pa;
			size_t elements = 0;
			while (pb < LP && elements + (size_t)(p.off[pb + 1] - p.off[pb]) <= capacity) elements += (size_t)(p.off[pb + 1] - p.off[pb]), pb++;
			// (pb > pa: capacity holds the largest plane)
			p.pa = pa; p.pb = pb; p.pass_off = p.off[pa];
			if (const int rc = gsr_check_hip(hipMemsetAsync(p.sums, 0, elements * 8, s), "hipMemsetAsync(hexplane sums)")) return rc;
			p.nent = 0;
			size_t lds = 0;
			bool direct = false;
			for (int fp = pa; fp < pb; fp++) {
				if (p.lds[fp]) {
					p.ent[p.nent++] = (unsigned char)fp;
					lds = std::max(lds, (size_t)(p.off[fp + 1] - p.off[fp]) / C * 4 * 8);
				} else direct = true;
			}
			int rc = GSR_OK;
			gsr_hp_variant(desc->D, [&](auto DD) {
				if (p.nent) {
					auto kernel = gsr_hp_grad_lds_kernel<DD()>;
					if (lds > 64 * 1024)
						rc = gsr_check_hip(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, GSR_HEXPLANE_LDS_BYTES),
						                   "hipFuncSetAttribute(hexplane)");
					if (rc) return;
					const long long tiles = ((long long)desc->N + GSR_HP_LDS_THREADS - 1) / GSR_HP_LDS_THREADS;
					hipEvent_t t0 = nullptr, t1 = nullptr;   // the two paths are single-kernel stages of their own when asked for by name
					gsr_prof_kernel_events(s, "hexplane_backward_lds", &t0, &t1);
					gsr_launch(kernel, dim3((unsigned)std::min<long long>(tiles, GSR_HP_LDS_GROUPS), C / 4, p.nent), dim3(GSR_HP_LDS_THREADS), lds, s, t0, t1, p);
				}
				if (direct) {
					p.l0 = pa / p.P;
					const int l1 = (pb - 1) / p.P;
					hipEvent_t t0 = nullptr, t1 = nullptr;
					gsr_prof_kernel_events(s, "hexplane_backward_direct", &t0, &t1);
					gsr_launch(gsr_hp_grad_direct_kernel<DD()>, dim3((unsigned)row_blocks, l1 - p.l0 + 1), dim3(256), 0, s, t0, t1, p);
				}
			});
			if (rc) return rc;
			hipLaunchKernelGGL(gsr_hp_convert_kernel, dim3(gsr_hp_blocks((long long)elements / (pb - pa), 1024), pb - pa), dim3(256), 0, s, p);
			pa = pb;
		}
	}
	return gsr_stage_done(s, 0, "hexplane_backward");
}

extern "C" int gsr_hexplane_regularizer(const gsr_hexplane_desc* desc, const float* table, float w_tv_space, float w_tv_time, float w_smooth_space,
                                        float w_smooth_time, float w_l1_time, float* value, float* dtable, void* scratch, size_t scratch_bytes, void* stream)
{
	const char* who = "gsr_hexplane_regularizer";
	if (const char* e = gsr_hp_shape_error(desc)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: %s", who, e);
	if (!table || !value) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: table or value is NULL", who);
	if (const int rc = gsr_hp_check_scratch(who, scratch, scratch_bytes, GSR_HEXPLANE_REG_SCRATCH_BYTES)) return rc;
	static_assert(GSR_HP_MAX_FLAT * GSR_HP_REG_BLOCKS * 8 <= GSR_HEXPLANE_REG_SCRATCH_BYTES, "the partial sums must fit the scratch");
	hipStream_t s = (hipStream_t)stream;
	GsrProfScope prof(s, "hexplane_regularizer");
	GsrHpParams p = gsr_hp_params(*desc);
	p.table = table; p.dtable = dtable;
	GsrHpReg w;
	w.tv[0] = w_tv_space; w.tv[1] = w_tv_time; w.smooth[0] = w_smooth_space; w.smooth[1] = w_smooth_time; w.l1 = w_l1_time;
	const int LP = p.L * p.P;
	hipLaunchKernelGGL(gsr_hp_reg_kernel, dim3(GSR_HP_REG_BLOCKS, LP), dim3(256), 0, s, p, w, desc->D, (double*)scratch);
	hipLaunchKernelGGL(gsr_hp_reg_fold_kernel, dim3(1), dim3(256), 0, s, (const double*)scratch, LP * GSR_HP_REG_BLOCKS, value);
	return gsr_stage_done(s, 0, "hexplane_regularizer");
}
