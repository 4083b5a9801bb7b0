// slice4d.hip -- 4D Gaussians conditioned on a time stamp (include/gsr_slice4d.h): the time slice with its backward, and the
// harmonic colour coefficients with theirs.
//
//   slice:     one thread per Gaussian, plain loads: a wave's rows are contiguous in every leaf, so its loads cover whole lines (the
//              (P,3) rows as three dword loads at a 12-byte stride, 768 contiguous bytes per wave; the quaternions as one 16-byte load
//              where the pointers allow it).  Everything is formed in double from the float32 leaves (gsr_slice4d_math.h) and rounded
//              once at the store.  The backward recomputes the forward's values and runs the hand-derived chain; a masked row
//              (g <= cutoff) writes +0 to every leaf gradient without reading the incoming ones.
//   harmonics: a workgroup owns GSR_HARM_ROWS consecutive Gaussians.  Its first wave forms the rows' coefficients
//              c_n = fp32(cos(2 pi n (time - t) / period)) once, in double, into the LDS; then all lanes walk the rows' 3 M floats,
//              which are contiguous per harmonic, four floats (16 bytes) per lane where 3 M is a multiple of four and the pointers
//              are aligned, one float otherwise.  shs is one fmaf chain in ascending n started at harmonic 0.  The backward writes
//              c_n g_shs and, for dL/dt, leaves each lane's part of sum_n (2 pi n / period) sin(...) <f_n, g_shs>, accumulated in
//              double in ascending n and element order, in the LDS; the row's own lane adds the parts in ascending order.  No atomics:
//              every output has one writer and a fixed order of evaluation.
// Row indices are 32-bit (api.hip refuses 6 P beyond that); offsets into features_t are 64-bit.
#include "gsr_internal.h"
#include "gsr_slice4d_math.h"
#include "../../include/gsr_slice4d.h"

#define GSR_S4D_THREADS GSR_SLICE4D_THREADS
#define GSR_HARM_ROWS 64      // Gaussians per workgroup of the harmonic kernels: one lane of the first wave each
#define GSR_HARM_MAX_M3 48    // 3 M at M = 16

template <bool Q16>
__device__ __forceinline__ void gsr_s4d_load(unsigned i, const float* __restrict__ xyz, const float* __restrict__ t, const float* __restrict__ scaling,
                                             const float* __restrict__ scaling_t, const float* __restrict__ rotation,
                                             const float* __restrict__ rotation_r, const float* __restrict__ opacity, GsrS4dLeaves& in)
{
#pragma unroll
	for (int k = 0; k < 3; k++) {
		in.xyz[k] = xyz[3 * i + k];
		in.ls[k] = scaling[3 * i + k];
	}
	in.t = t[i];
	in.ls[3] = scaling_t[i];
	in.o = opacity[i];
	if (Q16) {
		const float4 l = reinterpret_cast<const float4*>(rotation)[i], r = reinterpret_cast<const float4*>(rotation_r)[i];
		in.l[0] = l.x; in.l[1] = l.y; in.l[2] = l.z; in.l[3] = l.w;
		in.r[0] = r.x; in.r[1] = r.y; in.r[2] = r.z; in.r[3] = r.w;
	} else {
#pragma unroll
		for (int k = 0; k < 4; k++) {
			in.l[k] = rotation[4 * i + k];
			in.r[k] = rotation_r[4 * i + k];
		}
	}
}

template <bool Q16>
__global__ void __launch_bounds__(GSR_S4D_THREADS) gsr_slice4d_forward_kernel(unsigned P, const float* __restrict__ xyz, const float* __restrict__ t,
                                                                              const float* __restrict__ scaling, const float* __restrict__ scaling_t,
                                                                              const float* __restrict__ rotation, const float* __restrict__ rotation_r,
                                                                              const float* __restrict__ opacity, double time, double modifier,
                                                                              double cutoff, float* __restrict__ means3D, float* __restrict__ cov3D,
                                                                              float* __restrict__ opacities, float* __restrict__ velocity)
{
	const unsigned i = blockIdx.x * GSR_S4D_THREADS + threadIdx.x;
	if (i >= P) return;
	GsrS4dLeaves in;
	gsr_s4d_load<Q16>(i, xyz, t, scaling, scaling_t, rotation, rotation_r, opacity, in);
	GsrS4dEval v;
	gsr_s4d_eval(in, time, modifier, v);
	double vel[3];
#pragma unroll
	for (int k = 0; k < 3; k++) vel[k] = v.u[k] / v.stt;
	if (means3D) {
#pragma unroll
		for (int k = 0; k < 3; k++) means3D[3 * i + k] = (float)((double)in.xyz[k] + vel[k] * v.delta);
	}
	if (velocity) {
#pragma unroll
		for (int k = 0; k < 3; k++) velocity[3 * i + k] = (float)vel[k];
	}
	if (cov3D) {
		int n = 0;
#pragma unroll
		for (int a = 0; a < 3; a++) {
#pragma unroll
			for (int b = a; b < 3; b++, n++) cov3D[6 * i + n] = (float)(gsr_s4d_sigma11(v, a, b) - v.u[a] * v.u[b] / v.stt);
		}
	}
	if (opacities) opacities[i] = v.g > cutoff ? (float)(v.sig * v.g) : 0.0f;
}

template <bool Q16>
__global__ void __launch_bounds__(GSR_S4D_THREADS) gsr_slice4d_backward_kernel(gsr_slice4d_backward_args a)
{
	const unsigned i = blockIdx.x * GSR_S4D_THREADS + threadIdx.x;
	if (i >= (unsigned)a.P) return;
	GsrS4dLeaves in;
	gsr_s4d_load<Q16>(i, a.xyz, a.t, a.scaling, a.scaling_t, a.rotation, a.rotation_r, a.opacity, in);
	GsrS4dEval v;
	gsr_s4d_eval(in, a.time, a.modifier, v);
	GsrS4dGrads d;
	if (v.g > a.cutoff) {
		double gm[3], gc[6], gv[3];
#pragma unroll
		for (int k = 0; k < 3; k++) {
			gm[k] = a.g_means3D ? (double)a.g_means3D[3 * i + k] : 0.0;
			gv[k] = a.g_velocity ? (double)a.g_velocity[3 * i + k] : 0.0;
		}
#pragma unroll
		for (int k = 0; k < 6; k++) gc[k] = a.g_cov3D ? (double)a.g_cov3D[6 * i + k] : 0.0;
		const double go = a.g_opacities ? (double)a.g_opacities[i] : 0.0;
		gsr_s4d_chain(v, gm, gc, go, gv, d);
	} else {
#pragma unroll
		for (int k = 0; k < 4; k++) {
			d.ls[k] = 0.0;
			d.l[k] = 0.0;
			d.r[k] = 0.0;
		}
		d.xyz[0] = d.xyz[1] = d.xyz[2] = d.t = d.o = 0.0;
	}
	if (a.d_xyz) {
#pragma unroll
		for (int k = 0; k < 3; k++) a.d_xyz[3 * i + k] = (float)d.xyz[k];
	}
	if (a.d_t) a.d_t[i] = (float)d.t;
	if (a.d_scaling) {
#pragma unroll
		for (int k = 0; k < 3; k++) a.d_scaling[3 * i + k] = (float)d.ls[k];
	}
	if (a.d_scaling_t) a.d_scaling_t[i] = (float)d.ls[3];
	if (Q16) {
		if (a.d_rotation) reinterpret_cast<float4*>(a.d_rotation)[i] = make_float4((float)d.l[0], (float)d.l[1], (float)d.l[2], (float)d.l[3]);
		if (a.d_rotation_r) reinterpret_cast<float4*>(a.d_rotation_r)[i] = make_float4((float)d.r[0], (float)d.r[1], (float)d.r[2], (float)d.r[3]);
	} else {
#pragma unroll
		for (int k = 0; k < 4; k++) {
			if (a.d_rotation) a.d_rotation[4 * i + k] = (float)d.l[k];
			if (a.d_rotation_r) a.d_rotation_r[4 * i + k] = (float)d.r[k];
		}
	}
	if (a.d_opacity) a.d_opacity[i] = (float)d.o;
}

// ---- harmonic colour coefficients ----
template <int VEC> struct GsrHarmVec;
template <> struct GsrHarmVec<1> {
	float v[1];
	__device__ __forceinline__ void load(const float* p) { v[0] = *p; }
	__device__ __forceinline__ void store(float* p) const { *p = v[0]; }
};
template <> struct GsrHarmVec<4> {
	float v[4];
	__device__ __forceinline__ void load(const float* p)
	{
		const float4 x = *reinterpret_cast<const float4*>(p);
		v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
	}
	__device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// the argument of harmonic n, in double: 2 pi n (time - t) / period
__device__ __forceinline__ double gsr_harm_arg(int n, double delta, double period) { return 6.283185307179586 * (double)n * delta / period; }

template <int VEC>
__global__ void __launch_bounds__(GSR_S4D_THREADS) gsr_harmonic_forward_kernel(unsigned P, int N, unsigned M3, const float* __restrict__ features_t,
                                                                               const float* __restrict__ t, double time, double period,
                                                                               float* __restrict__ shs)
{
	__shared__ float coef[GSR_HARM_ROWS][4];
	const unsigned base = blockIdx.x * GSR_HARM_ROWS;
	const unsigned rows = min((unsigned)GSR_HARM_ROWS, P - base);
	if (threadIdx.x < rows) {
		const double delta = time - (double)t[base + threadIdx.x];
#pragma unroll
		for (int n = 1; n <= GSR_HARMONIC_MAX_N; n++) coef[threadIdx.x][n] = n <= N ? (float)cos(gsr_harm_arg(n, delta, period)) : 0.0f;
	}
	__syncthreads();
	const unsigned per = M3 / VEC, total = rows * per;
	for (unsigned e = threadIdx.x; e < total; e += GSR_S4D_THREADS) {
		const unsigned row = e / per, j = (e - row * per) * VEC;
		const size_t gi = (size_t)base + row;
		const float* src = features_t + gi * (size_t)(N + 1) * M3 + j;
		GsrHarmVec<VEC> acc;
		acc.load(src);
#pragma unroll
		for (int n = 1; n <= GSR_HARMONIC_MAX_N; n++) {
			if (n <= N) {
				GsrHarmVec<VEC> x;
				x.load(src + (size_t)n * M3);
				const float c = coef[row][n];
#pragma unroll
				for (int k = 0; k < VEC; k++) acc.v[k] = __builtin_fmaf(c, x.v[k], acc.v[k]);
			}
		}
		acc.store(shs + gi * M3 + j);
	}
}

template <int VEC>
__global__ void __launch_bounds__(GSR_S4D_THREADS) gsr_harmonic_backward_kernel(unsigned P, int N, unsigned M3, const float* __restrict__ features_t,
                                                                                const float* __restrict__ t, double time, double period,
                                                                                const float* __restrict__ g_shs, float* __restrict__ d_features_t,
                                                                                float* __restrict__ d_t)
{
	__shared__ float coef[GSR_HARM_ROWS][4];
	__shared__ double wsin[GSR_HARM_ROWS][4];
	__shared__ double part[GSR_HARM_ROWS * GSR_HARM_MAX_M3 / VEC];
	const unsigned base = blockIdx.x * GSR_HARM_ROWS;
	const unsigned rows = min((unsigned)GSR_HARM_ROWS, P - base);
	if (threadIdx.x < rows) {
		const double delta = time - (double)t[base + threadIdx.x];
#pragma unroll
		for (int n = 1; n <= GSR_HARMONIC_MAX_N; n++) {
			const double arg = gsr_harm_arg(n, delta, period);
			coef[threadIdx.x][n] = n <= N ? (float)cos(arg) : 0.0f;
			wsin[threadIdx.x][n] = n <= N ? (6.283185307179586 * (double)n / period) * sin(arg) : 0.0;
		}
	}
	__syncthreads();
	const unsigned per = M3 / VEC, total = rows * per;   // total <= GSR_HARM_ROWS * GSR_HARM_MAX_M3 / VEC: api.hip refuses M > 16
	for (unsigned e = threadIdx.x; e < total; e += GSR_S4D_THREADS) {
		const unsigned row = e / per, j = (e - row * per) * VEC;
		const size_t gi = (size_t)base + row;
		const size_t at = gi * (size_t)(N + 1) * M3 + j;
		GsrHarmVec<VEC> g;
		g.load(g_shs + gi * M3 + j);
		if (d_features_t) {
			g.store(d_features_t + at);
#pragma unroll
			for (int n = 1; n <= GSR_HARMONIC_MAX_N; n++) {
				if (n <= N) {
					const float c = coef[row][n];
					GsrHarmVec<VEC> o;
#pragma unroll
					for (int k = 0; k < VEC; k++) o.v[k] = c * g.v[k];
					o.store(d_features_t + at + (size_t)n * M3);
				}
			}
		}
		if (d_t) {
			double p = 0.0;
#pragma unroll
			for (int n = 1; n <= GSR_HARMONIC_MAX_N; n++) {
				if (n <= N) {
					GsrHarmVec<VEC> x;
					x.load(features_t + at + (size_t)n * M3);
					double dot = 0.0;
#pragma unroll
					for (int k = 0; k < VEC; k++) dot += (double)x.v[k] * (double)g.v[k];
					p += wsin[row][n] * dot;
				}
			}
			part[e] = p;
		}
	}
	__syncthreads();
	if (d_t && threadIdx.x < rows) {
		double s = 0.0;
		for (unsigned q = 0; q < per; q++) s += part[threadIdx.x * per + q];
		d_t[base + threadIdx.x] = (float)s;
	}
}

// ---- host side ----
static unsigned gsr_s4d_blocks(int P, int rows) { return (unsigned)(((long long)P + rows - 1) / rows); }
static bool gsr_s4d_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

void gsr_launch_slice4d_forward(int P, const float* xyz, const float* t, const float* scaling, const float* scaling_t, const float* rotation,
                                const float* rotation_r, const float* opacity, double time, double modifier, double cutoff, float* means3D,
                                float* cov3D, float* opacities, float* velocity, hipStream_t s)
{
	GsrProfScope p(s, "slice4d_forward");
	const dim3 grid(gsr_s4d_blocks(P, GSR_S4D_THREADS)), block(GSR_S4D_THREADS);
	if (gsr_s4d_aligned16(rotation) && gsr_s4d_aligned16(rotation_r))
		hipLaunchKernelGGL(gsr_slice4d_forward_kernel<true>, grid, block, 0, s, (unsigned)P, xyz, t, scaling, scaling_t, rotation, rotation_r, opacity,
		                   time, modifier, cutoff, means3D, cov3D, opacities, velocity);
	else
		hipLaunchKernelGGL(gsr_slice4d_forward_kernel<false>, grid, block, 0, s, (unsigned)P, xyz, t, scaling, scaling_t, rotation, rotation_r, opacity,
		                   time, modifier, cutoff, means3D, cov3D, opacities, velocity);
}

void gsr_launch_slice4d_backward(const gsr_slice4d_backward_args& a, hipStream_t s)
{
	GsrProfScope p(s, "slice4d_backward");
	const dim3 grid(gsr_s4d_blocks(a.P, GSR_S4D_THREADS)), block(GSR_S4D_THREADS);
	const bool q16 = gsr_s4d_aligned16(a.rotation) && gsr_s4d_aligned16(a.rotation_r) && gsr_s4d_aligned16(a.d_rotation) && gsr_s4d_aligned16(a.d_rotation_r);
	if (q16) hipLaunchKernelGGL(gsr_slice4d_backward_kernel<true>, grid, block, 0, s, a);
	else hipLaunchKernelGGL(gsr_slice4d_backward_kernel<false>, grid, block, 0, s, a);
}

void gsr_launch_harmonic_forward(int P, int N, int M, const float* features_t, const float* t, double time, double period, float* shs, hipStream_t s)
{
	GsrProfScope p(s, "harmonic_forward");
	const dim3 grid(gsr_s4d_blocks(P, GSR_HARM_ROWS)), block(GSR_S4D_THREADS);
	const unsigned M3 = 3u * (unsigned)M;
	if (M3 % 4 == 0 && gsr_s4d_aligned16(features_t) && gsr_s4d_aligned16(shs))
		hipLaunchKernelGGL(gsr_harmonic_forward_kernel<4>, grid, block, 0, s, (unsigned)P, N, M3, features_t, t, time, period, shs);
	else
		hipLaunchKernelGGL(gsr_harmonic_forward_kernel<1>, grid, block, 0, s, (unsigned)P, N, M3, features_t, t, time, period, shs);
}

void gsr_launch_harmonic_backward(int P, int N, int M, const float* features_t, const float* t, double time, double period, const float* g_shs,
                                  float* d_features_t, float* d_t, hipStream_t s)
{
	GsrProfScope p(s, "harmonic_backward");
	const dim3 grid(gsr_s4d_blocks(P, GSR_HARM_ROWS)), block(GSR_S4D_THREADS);
	const unsigned M3 = 3u * (unsigned)M;
	if (M3 % 4 == 0 && gsr_s4d_aligned16(features_t) && gsr_s4d_aligned16(g_shs) && gsr_s4d_aligned16(d_features_t))
		hipLaunchKernelGGL(gsr_harmonic_backward_kernel<4>, grid, block, 0, s, (unsigned)P, N, M3, features_t, t, time, period, g_shs, d_features_t, d_t);
	else
		hipLaunchKernelGGL(gsr_harmonic_backward_kernel<1>, grid, block, 0, s, (unsigned)P, N, M3, features_t, t, time, period, g_shs, d_features_t, d_t);
}
