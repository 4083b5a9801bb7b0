// mcmc.hip -- the mechanical pieces of fixed-budget (MCMC) training (include/gsr_mcmc.h): noise injection, relocation, regulariser.
//
//   noise:     one thread per Gaussian, plain loads (a wave's rows are contiguous in every tensor, so its loads cover whole lines):
//              56 B in, 12 B out.  Sigma n is formed as R (s^2 * (R^T n)), never as nine covariance entries.  The gate is evaluated in
//              double and rounded once; where its exponential would overflow in fp32 (o above about 0.89) it is exactly 0, as in the
//              stock fp32 sequence, and the row is left alone: no store, the bits stay.
//   relocate:  three kernels behind a memset of the counts.  (1) counts[src[j]] += 1: integer atomics, the only atomics of the file,
//              whose result does not depend on their order.  (2) one wave per entry: every lane evaluates the entry's new opacity and
//              scale ratio in double (the same for all lanes, so it costs the wave one evaluation), then the lanes walk the floats of
//              each group's row: reads of row src[j] as it was, writes to row dst[j] only.  (3) one wave per entry copies the new
//              logit and log-scales from row dst[j] to row src[j] -- entries that share a source write the same bits -- and zeroes
//              the source's moments.  dst and src are disjoint and dst has no duplicates (the caller's to keep), so no kernel reads
//              what another thread of the same launch writes.
//   reg:       elementwise over the logits and, flat, over the log-scales; value partials {opacity, scale} per workgroup in a fixed
//              order, one workgroup folds them in double precision (the order of gsr_bilagrid_tv_finalize_kernel).
// Indices are 32-bit: api.hip refuses sizes beyond that.  An entry whose row index lies outside [0, P) is skipped by all three
// relocation kernels.
#include "gsr_internal.h"
#include "../../include/gsr_mcmc.h"

#define GSR_MCMC_THREADS 256
#define GSR_MCMC_ENTRIES_PER_WG (GSR_MCMC_THREADS / 64)                          // relocation: one wave per entry
#define GSR_MCMC_REG_GAUSSIANS (GSR_MCMC_REG_ELEMS_PER_THREAD / 3)               // per thread: that many logits, three times as many scales
#define GSR_MCMC_REG_WG_GAUSSIANS (GSR_MCMC_REG_THREADS * GSR_MCMC_REG_GAUSSIANS)

__global__ void __launch_bounds__(GSR_MCMC_THREADS) gsr_mcmc_noise_kernel(unsigned P, float* __restrict__ xyz, const float* __restrict__ opacity,
                                                                          const float* __restrict__ scaling, const float* __restrict__ rotation,
                                                                          const float* __restrict__ noise, float scaler)
{
	const unsigned i = blockIdx.x * GSR_MCMC_THREADS + threadIdx.x;
	if (i >= P) return;
	// The gate multiplies the opacity by 100 inside an exponential: in fp32 the rounding of o alone costs it two digits (the stock
	// sequence: 1e-5).  Its two exponentials are taken in double from the logit, 1 - o = 1 / (1 + e^l), and the gate is rounded once.
	const double arg = -100.0 * (1.0 / (1.0 + exp((double)opacity[i])) - 0.995);
	if (arg > 88.72283905206835) return;   // log(FLT_MAX): where the fp32 exponential overflows the gate is exactly 0
	const float g = (float)((double)scaler / (1.0 + exp(arg)));
	const float n0 = noise[3 * i] * g, n1 = noise[3 * i + 1] * g, n2 = noise[3 * i + 2] * g;
	float q[4];
	const float qin[4] = {rotation[4 * i], rotation[4 * i + 1], rotation[4 * i + 2], rotation[4 * i + 3]};
	gsr_act_normalize4(qin, q);
	const GsrMat3 R = gsr_build_R(q[0], q[1], q[2], q[3]);
	const float s0 = gsr_act_exp(scaling[3 * i]), s1 = gsr_act_exp(scaling[3 * i + 1]), s2 = gsr_act_exp(scaling[3 * i + 2]);
	// t = s^2 * (R^T n)
	const float t0 = (s0 * s0) * (R.m[0][0] * n0 + R.m[1][0] * n1 + R.m[2][0] * n2);
	const float t1 = (s1 * s1) * (R.m[0][1] * n0 + R.m[1][1] * n1 + R.m[2][1] * n2);
	const float t2 = (s2 * s2) * (R.m[0][2] * n0 + R.m[1][2] * n1 + R.m[2][2] * n2);
	// the displacement is complete before it meets the position: xyz + d with d the value an xyz of zero would receive
	const float d0 = R.m[0][0] * t0 + R.m[0][1] * t1 + R.m[0][2] * t2;
	const float d1 = R.m[1][0] * t0 + R.m[1][1] * t1 + R.m[1][2] * t2;
	const float d2 = R.m[2][0] * t0 + R.m[2][1] * t1 + R.m[2][2] * t2;
	xyz[3 * i] += d0;
	xyz[3 * i + 1] += d1;
	xyz[3 * i + 2] += d2;
}

// ---- relocation ----
struct GsrMcmcTable {
	float* param[GSR_ADAM_MAX_GROUPS];
	float* exp_avg[GSR_ADAM_MAX_GROUPS];
	float* exp_avg_sq[GSR_ADAM_MAX_GROUPS];
	unsigned row[GSR_ADAM_MAX_GROUPS];
	int ngroups, opacity_group, scale_group;
};

__device__ __forceinline__ bool gsr_mcmc_entry(unsigned j, unsigned P, const int64_t* __restrict__ dst, const int64_t* __restrict__ src, unsigned& d,
                                               unsigned& s)
{
	const int64_t dj = dst[j], sj = src[j];
	if (dj < 0 || dj >= (int64_t)P || sj < 0 || sj >= (int64_t)P) return false;
	d = (unsigned)dj; s = (unsigned)sj;
	return true;
}

__global__ void __launch_bounds__(GSR_MCMC_THREADS) gsr_mcmc_count_kernel(unsigned D, unsigned P, const int64_t* __restrict__ dst,
                                                                          const int64_t* __restrict__ src, int* __restrict__ counts)
{
	const unsigned j = blockIdx.x * GSR_MCMC_THREADS + threadIdx.x;
	unsigned d, s;
	if (j >= D || !gsr_mcmc_entry(j, P, dst, src, d, s)) return;
	atomicAdd(&counts[s], 1);
}

// new logit and log(o / denom) of a source with logit l named by n entries (1 <= n <= GSR_MCMC_MAX_RATIO), in double.
// 1 - o = 1 / (1 + e^l), so o' = 1 - (1 - o)^(1/n) = -expm1(-log1p(e^l) / n) without the cancellation of either subtraction;
// denom in its collapsed form, C(n, k + 1) by the exact recurrence C(n, k + 2) = C(n, k + 1) (n - k - 1) / (k + 2) (every product stays
// below 2^53 for n <= 51, every quotient is an integer).
__device__ __forceinline__ void gsr_mcmc_rescale(double l, int n, double min_opacity, float& new_logit, double& log_ratio)
{
	const double o = 1.0 / (1.0 + exp(-l));
	const double on = -expm1(-log1p(exp(l)) / (double)n);
	double denom = 0.0, c = (double)n, p = on;   // C(n, k + 1), (-1)^k o'^(k + 1)
	for (int k = 0; k < n; k++) {
		denom += c * p / sqrt((double)(k + 1));
		c = c * (double)(n - k - 1) / (double)(k + 2);
		p *= -on;
	}
	const double oc = fmin(fmax(on, min_opacity), 1.0 - 1.1920928955078125e-07);   // 1 - 2^-23
	new_logit = (float)(log(oc) - log1p(-oc));
	log_ratio = log(o / denom);
}

__global__ void __launch_bounds__(GSR_MCMC_THREADS) gsr_mcmc_move_kernel(unsigned D, unsigned P, GsrMcmcTable t, const int64_t* __restrict__ dst,
                                                                         const int64_t* __restrict__ src, const int* __restrict__ counts,
                                                                         double min_opacity)
{
	const unsigned j = blockIdx.x * GSR_MCMC_ENTRIES_PER_WG + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	unsigned d, s;
	if (j >= D || !gsr_mcmc_entry(j, P, dst, src, d, s)) return;
	const int n = min(GSR_MCMC_MAX_RATIO, 1 + counts[s]);
	float new_logit;
	double log_ratio;
	gsr_mcmc_rescale((double)t.param[t.opacity_group][s], n, min_opacity, new_logit, log_ratio);
	for (int g = 0; g < t.ngroups; g++) {
		float* p = t.param[g];
		const unsigned row = t.row[g];
		if (g == t.opacity_group) {
			if (lane == 0) p[d] = new_logit;
		} else if (g == t.scale_group) {
			if (lane < 3) p[3 * d + lane] = (float)((double)p[3 * s + lane] + log_ratio);   // log((o / denom) exp(log_scale))
		} else {
			for (unsigned f = lane; f < row; f += 64) p[d * row + f] = p[s * row + f];
		}
	}
}

__global__ void __launch_bounds__(GSR_MCMC_THREADS) gsr_mcmc_source_kernel(unsigned D, unsigned P, GsrMcmcTable t, const int64_t* __restrict__ dst,
                                                                           const int64_t* __restrict__ src, int zero_moments)
{
	const unsigned j = blockIdx.x * GSR_MCMC_ENTRIES_PER_WG + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	unsigned d, s;
	if (j >= D || !gsr_mcmc_entry(j, P, dst, src, d, s)) return;
	if (lane == 0) t.param[t.opacity_group][s] = t.param[t.opacity_group][d];
	if (lane < 3) t.param[t.scale_group][3 * s + lane] = t.param[t.scale_group][3 * d + lane];
	if (!zero_moments) return;
	for (int g = 0; g < t.ngroups; g++) {
		if (!t.exp_avg[g]) continue;
		const unsigned row = t.row[g];
		for (unsigned f = lane; f < row; f += 64) {
			t.exp_avg[g][s * row + f] = 0.0f;
			t.exp_avg_sq[g][s * row + f] = 0.0f;
		}
	}
}

// ---- regulariser ----
// partial[blockIdx.x] = {sum sigmoid(l), sum exp(s)} of the workgroup's Gaussians.  The exponentials are fp32; the rational part of the
// sigmoid and the products with the coefficients are formed in double and rounded once, so that an element carries the exponential's
// error and one rounding.  co = w_o / P, cs = w_s / (3 P).
__global__ void __launch_bounds__(GSR_MCMC_REG_THREADS) gsr_mcmc_reg_kernel(unsigned P, double co, double cs, const float* __restrict__ opacity,
                                                                            const float* __restrict__ scaling, float* __restrict__ d_opacity,
                                                                            float* __restrict__ d_scaling, float2* __restrict__ partial)
{
	__shared__ float wsum[GSR_MCMC_REG_THREADS / 64][2];
	const unsigned n3 = 3u * P;
	float qo = 0.f, qs = 0.f;
#pragma unroll
	for (int k = 0; k < GSR_MCMC_REG_GAUSSIANS; k++) {
		const unsigned i = blockIdx.x * GSR_MCMC_REG_WG_GAUSSIANS + k * GSR_MCMC_REG_THREADS + threadIdx.x;
		if (i >= P) continue;
		const float l = opacity[i];
		const double e = (double)expf(-fabsf(l));        // <= 1
		const double big = 1.0 / (1.0 + e), small = e * big;   // sigmoid(|l|), sigmoid(-|l|)
		qo += (float)(l >= 0.f ? big : small);
		if (d_opacity) d_opacity[i] = (float)(co * (big * small));   // sigmoid(l) sigmoid(-l)
	}
#pragma unroll
	for (int k = 0; k < GSR_MCMC_REG_ELEMS_PER_THREAD; k++) {
		const unsigned i = blockIdx.x * (3 * GSR_MCMC_REG_WG_GAUSSIANS) + k * GSR_MCMC_REG_THREADS + threadIdx.x;
		if (i >= n3) continue;
		const float x = expf(scaling[i]);
		qs += x;
		if (d_scaling) d_scaling[i] = (float)(cs * (double)x);
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		qo += __shfl_down(qo, off, 64);
		qs += __shfl_down(qs, off, 64);
	}
	if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6][0] = qo; wsum[threadIdx.x >> 6][1] = qs; }
	__syncthreads();
	if (threadIdx.x == 0)   // the waves as a tree as well: log2(GSR_MCMC_REG_THREADS) levels in all
		partial[blockIdx.x] = make_float2((wsum[0][0] + wsum[1][0]) + (wsum[2][0] + wsum[3][0]), (wsum[0][1] + wsum[1][1]) + (wsum[2][1] + wsum[3][1]));
}

__global__ void __launch_bounds__(256) gsr_mcmc_reg_finalize_kernel(const float2* __restrict__ partial, int n, double co, double cs, float* __restrict__ val)
{
	__shared__ double sw[4][2];
	double v[2] = {0.0, 0.0};
	for (int i = threadIdx.x; i < n; i += 256) { const float2 p = partial[i]; v[0] += p.x; v[1] += p.y; }
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		v[0] += __shfl_down(v[0], off, 64);
		v[1] += __shfl_down(v[1], off, 64);
	}
	if ((threadIdx.x & 63) == 0) { sw[threadIdx.x >> 6][0] = v[0]; sw[threadIdx.x >> 6][1] = v[1]; }
	__syncthreads();
	if (threadIdx.x == 0)
		val[0] = (float)((sw[0][0] + sw[1][0] + sw[2][0] + sw[3][0]) * co + (sw[0][1] + sw[1][1] + sw[2][1] + sw[3][1]) * cs);
}

// ---- host side ----
static long long gsr_mcmc_noise_blocks(int P) { return ((long long)P + GSR_MCMC_THREADS - 1) / GSR_MCMC_THREADS; }
long long gsr_mcmc_relocate_blocks(int D) { return ((long long)D + GSR_MCMC_ENTRIES_PER_WG - 1) / GSR_MCMC_ENTRIES_PER_WG; }
static long long gsr_mcmc_reg_blocks(int P) { return ((long long)P + GSR_MCMC_REG_WG_GAUSSIANS - 1) / GSR_MCMC_REG_WG_GAUSSIANS; }
size_t gsr_mcmc_reg_scratch_size(int P) { return gsr_align_up((size_t)gsr_mcmc_reg_blocks(P) * sizeof(float2)); }

void gsr_launch_mcmc_noise(int P, float* xyz, const float* opacity, const float* scaling, const float* rotation, const float* noise, float scaler,
                           hipStream_t s)
{
	GsrProfScope p(s, "mcmc_noise");
	hipLaunchKernelGGL(gsr_mcmc_noise_kernel, dim3((unsigned)gsr_mcmc_noise_blocks(P)), dim3(GSR_MCMC_THREADS), 0, s, (unsigned)P, xyz, opacity, scaling,
	                   rotation, noise, scaler);
}

int gsr_launch_mcmc_relocate(const gsr_mcmc_relocate_args& a, hipStream_t s)
{
	GsrProfScope p(s, "mcmc_relocate");
	GsrMcmcTable t = {};
	t.ngroups = a.ngroups; t.opacity_group = a.opacity_group; t.scale_group = a.scale_group;
	for (int g = 0; g < a.ngroups; g++) {
		t.param[g] = a.groups[g].param; t.exp_avg[g] = a.groups[g].exp_avg; t.exp_avg_sq[g] = a.groups[g].exp_avg_sq;
		t.row[g] = (unsigned)a.groups[g].row;
	}
	const hipError_t e = hipMemsetAsync(a.counts, 0, (size_t)a.P * sizeof(int32_t), s);
	if (e != hipSuccess) return gsr_check_hip(e, "gsr_mcmc_relocate: memset of counts");
	const unsigned D = (unsigned)a.D, P = (unsigned)a.P, waves = (unsigned)gsr_mcmc_relocate_blocks(a.D);
	hipLaunchKernelGGL(gsr_mcmc_count_kernel, dim3((D + GSR_MCMC_THREADS - 1) / GSR_MCMC_THREADS), dim3(GSR_MCMC_THREADS), 0, s, D, P, a.dst, a.src,
	                   (int*)a.counts);
	hipLaunchKernelGGL(gsr_mcmc_move_kernel, dim3(waves), dim3(GSR_MCMC_THREADS), 0, s, D, P, t, a.dst, a.src, (const int*)a.counts,
	                   (double)a.min_opacity);
	hipLaunchKernelGGL(gsr_mcmc_source_kernel, dim3(waves), dim3(GSR_MCMC_THREADS), 0, s, D, P, t, a.dst, a.src, a.zero_src_moments);
	return GSR_OK;
}

void gsr_launch_mcmc_regularizer(int P, const float* opacity, const float* scaling, float w_o, float w_s, float* val, float* dL_dopacity,
                                 float* dL_dscaling, void* scratch, hipStream_t s)
{
	GsrProfScope p(s, "mcmc_reg");
	const unsigned blocks = (unsigned)gsr_mcmc_reg_blocks(P);
	const double co = (double)w_o / (double)P, cs = (double)w_s / (3.0 * (double)P);
	hipLaunchKernelGGL(gsr_mcmc_reg_kernel, dim3(blocks), dim3(GSR_MCMC_REG_THREADS), 0, s, (unsigned)P, co, cs, opacity, scaling, dL_dopacity,
	                   dL_dscaling, (float2*)scratch);
	hipLaunchKernelGGL(gsr_mcmc_reg_finalize_kernel, dim3(1), dim3(256), 0, s, (const float2*)scratch, (int)blocks, co, cs, val);
}
