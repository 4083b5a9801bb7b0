// filter3d.hip -- Mip-Splatting's 3D smoothing filter (include/gsr_filter3d.h): the camera sweep, the filtered activations with their
// backward, the baked leaves and the opacity reset.
//
//   sweep:     one thread per Gaussian keeps its position in registers and walks all C camera records.  The record's address depends
//              on the loop counter alone, so it is wave-uniform and the compiler fetches the 80 bytes with scalar loads: the loop is
//              vector-ALU work only, 31 instructions (three dot products as fma chains, two products with the focal lengths, the four
//              bounds, four differences, their smallest, two comparisons and a conditional min).  The frustum test has no quotient:
//              p_z > 0.2 where it counts, so lo <= p_x / p_z fx + cx is evaluated as 0 <= p_x fx - (lo - cx) p_z, one fma whose sign is
//              that of the exact difference.  Lanes behind the last Gaussian walk the cameras with the
//              last Gaussian's position, so that the workgroup reaches its barrier as a whole; they write nothing.
//              The thread writes its d (0: valid in no camera; a valid d exceeds 0) to `filter`, the workgroup its largest d to
//              scratch[4 + blockIdx.x].
//   fold:      one workgroup: scratch[0] = the largest partial (0: no row is valid anywhere), scratch[1] = f_max.
//   finish:    one thread per Gaussian: d, or scratch[0] where d is 0, becomes the filter; 100000 everywhere where scratch[0] is 0.
//   min and max are exact and commutative: no result depends on the order of the cameras or on how the rows fall into workgroups.
//   activate:  elementwise, plain loads (a wave's rows are contiguous in every tensor, so its loads cover whole lines).  Every value
//              is formed in double from the float32 inputs -- exponentials included: the per-axis ratios s_k / sqrt(s_k^2 + f^2), their
//              product and the sigmoid carry one rounding, the one to float32 at the store.  Forward, baked leaves, backward and reset
//              share one evaluation (gsr_f3d_eval).
// Indices are 32-bit: api.hip refuses sizes beyond that.
#include "gsr_internal.h"
#include "../../include/gsr_filter3d.h"

#define GSR_F3D_THREADS GSR_FILTER3D_THREADS
#define GSR_F3D_WAVES (GSR_F3D_THREADS / 64)
#define GSR_F3D_HEAD 4   // floats in front of the partial maxima: {largest d, f_max, -, -}

// the largest value of a workgroup, in thread 0 (every value is >= 0)
__device__ __forceinline__ float gsr_f3d_block_max(float v, float* wmax)
{
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
	if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = v;
	__syncthreads();
	float m = wmax[0];
#pragma unroll
	for (int w = 1; w < GSR_F3D_WAVES; w++) m = fmaxf(m, wmax[w]);
	return m;
}

template <bool PER_CAMERA>
__global__ void __launch_bounds__(GSR_F3D_THREADS) gsr_filter3d_sweep_kernel(unsigned P, int C, const float* __restrict__ xyz,
                                                                             const gsr_filter3d_camera* __restrict__ cameras,
                                                                             float* __restrict__ dist, float* __restrict__ partial)
{
	__shared__ float wmax[GSR_F3D_WAVES];
	const unsigned i = blockIdx.x * GSR_F3D_THREADS + threadIdx.x;
	const bool live = i < P;
	const unsigned j = live ? i : P - 1;
	const float x = xyz[3 * j], y = xyz[3 * j + 1], z = xyz[3 * j + 2];
	float d = INFINITY;
	for (int c = 0; c < C; c++) {
		const gsr_filter3d_camera& k = cameras[c];   // wave-uniform
		const float pz = fmaf(k.R[6], x, fmaf(k.R[7], y, fmaf(k.R[8], z, k.t[2])));
		const float u = fmaf(k.R[0], x, fmaf(k.R[1], y, fmaf(k.R[2], z, k.t[0]))) * k.fx;
		const float v = fmaf(k.R[3], x, fmaf(k.R[4], y, fmaf(k.R[5], z, k.t[1]))) * k.fy;
		// the four bounds as one sign: the smallest of u - lo p_z, hi p_z - u and the same in y; each difference is one fma, whose sign
		// is that of the exact difference.  One straight-line body, no branch per bound; a NaN is valid nowhere
		const float inside = fminf(fminf(fmaf(-fmaf(-0.15f, k.W, -k.cx), pz, u), fmaf(fmaf(1.15f, k.W, -k.cx), pz, -u)),
		                           fminf(fmaf(-fmaf(-0.15f, k.H, -k.cy), pz, v), fmaf(fmaf(1.15f, k.H, -k.cy), pz, -v)));
		const bool valid = (pz > 0.2f) & (inside >= 0.0f);
		const float cand = PER_CAMERA ? pz / k.fx : pz;
		d = valid ? fminf(d, cand) : d;
	}
	const float mine = live && d < INFINITY ? d : 0.0f;
	if (live) dist[i] = mine;
	const float m = gsr_f3d_block_max(mine, wmax);
	if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

__global__ void __launch_bounds__(GSR_F3D_THREADS) gsr_filter3d_fold_kernel(int n, int C, const gsr_filter3d_camera* __restrict__ cameras,
                                                                            float* __restrict__ scratch)
{
	__shared__ float wmax[2][GSR_F3D_WAVES];
	float dmax = 0.0f, fmax = 0.0f;
	for (int b = threadIdx.x; b < n; b += GSR_F3D_THREADS) dmax = fmaxf(dmax, scratch[GSR_F3D_HEAD + b]);
	for (int c = threadIdx.x; c < C; c += GSR_F3D_THREADS) fmax = fmaxf(fmax, cameras[c].fx);
	dmax = gsr_f3d_block_max(dmax, wmax[0]);
	fmax = gsr_f3d_block_max(fmax, wmax[1]);
	if (threadIdx.x == 0) { scratch[0] = dmax; scratch[1] = fmax; }
}

template <bool PER_CAMERA>
__global__ void __launch_bounds__(GSR_F3D_THREADS) gsr_filter3d_finish_kernel(unsigned P, const float* __restrict__ head, float* __restrict__ filter)
{
	const unsigned i = blockIdx.x * GSR_F3D_THREADS + threadIdx.x;
	if (i >= P) return;
	const float dmax = head[0], fmax = head[1];
	const float own = filter[i];
	const float d = own > 0.0f ? own : dmax;
	const float root = (float)0.4472135954999579;   // fp32(sqrt(0.2))
	float out = PER_CAMERA ? d * root : (d / fmax) * root;
	if (!(dmax > 0.0f)) out = GSR_FILTER3D_UNSEEN;
	filter[i] = out;
}

// ---- activations ----
// everything the four elementwise kernels need of one Gaussian, in double: sigmoid(|l|) and sigmoid(-|l|) from one exponential,
// s_k^2 + f^2, its root, and coef = prod_k s_k / root_k (each factor in [0, 1]: no overflow, and underflow only below 1e-308)
struct GsrF3dEval {
	double big, small, sig, ff, coef;
	double a[3], b[3], root[3];
};

__device__ __forceinline__ void gsr_f3d_sigmoid(float l, GsrF3dEval& v)
{
	const double e = exp(-fabs((double)l));   // <= 1
	v.big = 1.0 / (1.0 + e);
	v.small = e * v.big;
	v.sig = l >= 0.0f ? v.big : v.small;
}

__device__ __forceinline__ void gsr_f3d_axes(const float* __restrict__ ls, float f, GsrF3dEval& v)
{
	v.ff = (double)f * (double)f;
	v.coef = 1.0;
#pragma unroll
	for (int k = 0; k < 3; k++) {
		const double s = exp((double)ls[k]);
		v.a[k] = s * s;
		v.b[k] = v.a[k] + v.ff;
		v.root[k] = sqrt(v.b[k]);
		v.coef *= s / v.root[k];
	}
}

// BAKED: logit(opacities) and log(scales) in place of opacities and scales
template <bool BAKED>
__global__ void __launch_bounds__(GSR_F3D_THREADS) gsr_filter3d_activate_kernel(unsigned P, const float* __restrict__ opacity,
                                                                                const float* __restrict__ scaling, const float* __restrict__ filter,
                                                                                float* __restrict__ out_o, float* __restrict__ out_s)
{
	const unsigned i = blockIdx.x * GSR_F3D_THREADS + threadIdx.x;
	if (i >= P) return;
	const float l = opacity[i];
	const float ls[3] = {scaling[3 * i], scaling[3 * i + 1], scaling[3 * i + 2]};
	GsrF3dEval v;
	gsr_f3d_sigmoid(l, v);
	gsr_f3d_axes(ls, filter[i], v);
	const double o = v.sig * v.coef;
	if (out_o) {
		// 1 - o = sigmoid(-l) + sigmoid(l) (1 - coef): no cancellation against 1 where the logit is large
		if (BAKED) out_o[i] = (float)(log(o) - log((l >= 0.0f ? v.small : v.big) + v.sig * (1.0 - v.coef)));
		else out_o[i] = (float)o;
	}
	if (out_s) {
#pragma unroll
		for (int k = 0; k < 3; k++) out_s[3 * i + k] = BAKED ? (float)(0.5 * log(v.b[k])) : (float)v.root[k];
	}
}

__global__ void __launch_bounds__(GSR_F3D_THREADS) gsr_filter3d_activate_backward_kernel(unsigned P, const float* __restrict__ opacity,
                                                                                         const float* __restrict__ scaling,
                                                                                         const float* __restrict__ filter,
                                                                                         const float* __restrict__ g_opacities,
                                                                                         const float* __restrict__ g_scales,
                                                                                         float* __restrict__ d_opacity, float* __restrict__ d_scaling)
{
	const unsigned i = blockIdx.x * GSR_F3D_THREADS + threadIdx.x;
	if (i >= P) return;
	const float l = opacity[i];
	const float ls[3] = {scaling[3 * i], scaling[3 * i + 1], scaling[3 * i + 2]};
	GsrF3dEval v;
	gsr_f3d_sigmoid(l, v);
	gsr_f3d_axes(ls, filter[i], v);
	const double go = g_opacities ? (double)g_opacities[i] : 0.0;
	if (d_opacity) d_opacity[i] = (float)(go * (v.big * v.small) * v.coef);
	if (d_scaling) {
		const double through_opacity = go * (v.sig * v.coef);
#pragma unroll
		for (int k = 0; k < 3; k++) {
			const double gs = g_scales ? (double)g_scales[3 * i + k] : 0.0;
			d_scaling[3 * i + k] = (float)(gs * (v.a[k] / v.root[k]) + through_opacity * (v.ff / v.b[k]));
		}
	}
}

__global__ void __launch_bounds__(GSR_F3D_THREADS) gsr_filter3d_reset_kernel(unsigned P, float* __restrict__ opacity, const float* __restrict__ scaling,
                                                                             const float* __restrict__ filter, double max_opacity,
                                                                             float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq)
{
	const unsigned i = blockIdx.x * GSR_F3D_THREADS + threadIdx.x;
	if (i >= P) return;
	if (exp_avg) { exp_avg[i] = 0.0f; exp_avg_sq[i] = 0.0f; }
	const float l = opacity[i];
	GsrF3dEval v;
	gsr_f3d_sigmoid(l, v);
	if (!(v.sig > max_opacity)) return;   // coef <= 1: the cap is at least max_opacity, the row keeps its bits and its scales are not read
	const float ls[3] = {scaling[3 * i], scaling[3 * i + 1], scaling[3 * i + 2]};
	gsr_f3d_axes(ls, filter[i], v);
	const double cap = max_opacity / v.coef;   // +inf where coef is 0
	if (!(v.sig > cap)) return;                // cap < sig < 1 from here on
	opacity[i] = (float)(log(cap) - log1p(-cap));
}

// ---- host side ----
static unsigned gsr_f3d_blocks(int P) { return (unsigned)(((long long)P + GSR_F3D_THREADS - 1) / GSR_F3D_THREADS); }
size_t gsr_filter3d_scratch_size(int P) { return gsr_align_up(((size_t)GSR_F3D_HEAD + gsr_f3d_blocks(P)) * sizeof(float)); }

void gsr_launch_filter3d_sweep(int P, int C, const float* xyz, const gsr_filter3d_camera* cameras, int per_camera, float* filter, void* scratch,
                               hipStream_t s)
{
	GsrProfScope p(s, "filter3d_sweep");
	const unsigned blocks = gsr_f3d_blocks(P);
	float* head = (float*)scratch;
	if (per_camera) {
		hipLaunchKernelGGL(gsr_filter3d_sweep_kernel<true>, dim3(blocks), dim3(GSR_F3D_THREADS), 0, s, (unsigned)P, C, xyz, cameras, filter, head + GSR_F3D_HEAD);
		hipLaunchKernelGGL(gsr_filter3d_fold_kernel, dim3(1), dim3(GSR_F3D_THREADS), 0, s, (int)blocks, C, cameras, head);
		hipLaunchKernelGGL(gsr_filter3d_finish_kernel<true>, dim3(blocks), dim3(GSR_F3D_THREADS), 0, s, (unsigned)P, (const float*)head, filter);
	} else {
		hipLaunchKernelGGL(gsr_filter3d_sweep_kernel<false>, dim3(blocks), dim3(GSR_F3D_THREADS), 0, s, (unsigned)P, C, xyz, cameras, filter, head + GSR_F3D_HEAD);
		hipLaunchKernelGGL(gsr_filter3d_fold_kernel, dim3(1), dim3(GSR_F3D_THREADS), 0, s, (int)blocks, C, cameras, head);
		hipLaunchKernelGGL(gsr_filter3d_finish_kernel<false>, dim3(blocks), dim3(GSR_F3D_THREADS), 0, s, (unsigned)P, (const float*)head, filter);
	}
}

void gsr_launch_filter3d_activate(int P, const float* opacity, const float* scaling, const float* filter, float* out_o, float* out_s, int baked,
                                  hipStream_t s)
{
	GsrProfScope p(s, "filter3d_activate");
	if (baked)
		hipLaunchKernelGGL(gsr_filter3d_activate_kernel<true>, dim3(gsr_f3d_blocks(P)), dim3(GSR_F3D_THREADS), 0, s, (unsigned)P, opacity, scaling, filter, out_o, out_s);
	else
		hipLaunchKernelGGL(gsr_filter3d_activate_kernel<false>, dim3(gsr_f3d_blocks(P)), dim3(GSR_F3D_THREADS), 0, s, (unsigned)P, opacity, scaling, filter, out_o, out_s);
}

void gsr_launch_filter3d_activate_backward(int P, const float* opacity, const float* scaling, const float* filter, const float* g_opacities,
                                           const float* g_scales, float* d_opacity, float* d_scaling, hipStream_t s)
{
	GsrProfScope p(s, "filter3d_activate_bwd");
	hipLaunchKernelGGL(gsr_filter3d_activate_backward_kernel, dim3(gsr_f3d_blocks(P)), dim3(GSR_F3D_THREADS), 0, s, (unsigned)P, opacity, scaling, filter,
	                   g_opacities, g_scales, d_opacity, d_scaling);
}

void gsr_launch_filter3d_reset(int P, float* opacity, const float* scaling, const float* filter, double max_opacity, float* exp_avg, float* exp_avg_sq,
                               hipStream_t s)
{
	GsrProfScope p(s, "filter3d_reset");
	hipLaunchKernelGGL(gsr_filter3d_reset_kernel, dim3(gsr_f3d_blocks(P)), dim3(GSR_F3D_THREADS), 0, s, (unsigned)P, opacity, scaling, filter, max_opacity,
	                   exp_avg, exp_avg_sq);
}
