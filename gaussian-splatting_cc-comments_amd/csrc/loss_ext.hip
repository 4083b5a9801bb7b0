// loss_ext.hip -- the fused training loss with a pixel mask, a per-image exposure and an inverse-depth term (include/gsr_loss_ext.h).
//
// The structure is loss.hip's: a 64x32 tile with a 5-pixel halo, the window means built separably by the shared passes of
// gsr_loss_tile.h, three partial-derivative maps in scratch, one forward kernel, one backward kernel, one fold.  What is new happens
// at the two ends of a kernel and leaves the passes alone:
//   forward:  x'' = m (E x + b) and y'' = m y are formed WHILE STAGING, so sx / sy hold them and the halo outside the image is 0 (not
//             the exposure's bias, not m times anything).  With exposure a channel's workgroup reads the three raw planes of its tile
//             and halo; neither the mask nor the raw planes take LDS.  The channel-0 workgroups also do their tile's pixels of the
//             depth term (elementwise: value summed into a third partial, gradient written at once).
//   backward: without exposure one workgroup per tile and channel, as loss.hip.  With exposure dL/dimg_k needs all three G_c, so
//             one workgroup walks the three channels of its tile, keeps 4 pixels x 3 channels of dL/dimg in registers, and its
//             twelve exposure sums come from the same registers (four live at a time: channel c gives E[0..2][c] and E[c][3]).
//   fold:     value partials and exposure partials, in double, in a fixed order.
// The variants are template instantiations on (mask, exposure, depth): an absent option costs no load and no instruction.
#include "gsr_loss_tile.h"
#include "../../include/gsr_loss_ext.h"

#define GSR_LOSS_WAVES (GSR_LOSS_THREADS / 64)

struct GsrLossExtForward {
	int H, W;
	const float *img, *gt, *mask, *exposure, *invdepth, *prior, *dmask;
	float depth_scale;   // w / (H W)
	GsrLossTaps taps;
	float *dm, *d11, *d12, *dL_dinvdepth;
	float4* partial;     // per tile {sum |x'' - y''|, sum SSIM, sum |(d - d*) k|, 0}
};

struct GsrLossExtBackward {   // the exposure variant's arguments (C == 3)
	int H, W;
	const float *img, *gt, *mask, *exposure;
	GsrLossTaps taps;
	const float *dm, *d11, *d12;
	float lambda;
	float* dL_dimg;
	float* epart;        // per tile the twelve sums in dL_dexposure's order, or NULL
};

// column c of the colour transform: x'_c = e[0] x_0 + e[1] x_1 + e[2] x_2 + e[3].  Written out as one chain of FMAs so that the
// forward's staging and the backward's own pixels get the same bits.
__device__ __forceinline__ void gsr_exposure_column(const float* __restrict__ E, int c, float (&e)[4])
{
	e[0] = E[c]; e[1] = E[4 + c]; e[2] = E[8 + c]; e[3] = E[4 * c + 3];
}
__device__ __forceinline__ float gsr_expose(const float (&e)[4], float x0, float x1, float x2)
{
	return __builtin_fmaf(e[2], x2, __builtin_fmaf(e[1], x1, __builtin_fmaf(e[0], x0, e[3])));
}

// gsr_loss_stage for the forward: x'' and y'' of channel c, zero outside the image.  img: plane c without exposure, plane 0 with it.
template <bool MASK, bool EXPO>
__device__ __forceinline__ void gsr_loss_ext_stage(const float* __restrict__ img, const float* __restrict__ gt, const float* __restrict__ mask,
                                                   size_t plane, const float (&e)[4], int H, int W, int x0, int y0, float* sx, float* sy)
{
	constexpr int N = GSR_LOSS_HY * GSR_LOSS_HX, IT = (N + GSR_LOSS_THREADS - 1) / GSR_LOSS_THREADS, NX = EXPO ? 3 : 1;
	float xv[NX][IT], yv[IT], mv[IT];
#pragma unroll
	for (int k = 0; k < IT; k++) {
		const int i = threadIdx.x + k * GSR_LOSS_THREADS;
		const int r = i / GSR_LOSS_HX, q = i % GSR_LOSS_HX;
		const int gy = y0 + r, gx = x0 + q;
		const bool in = i < N && gy >= 0 && gy < H && gx >= 0 && gx < W;
		const size_t o = in ? (size_t)gy * W + gx : 0;
#pragma unroll
		for (int p = 0; p < NX; p++) xv[p][k] = img[p * plane + o];
		yv[k] = gt[o];
		mv[k] = MASK ? mask[o] : 1.f;
	}
#pragma unroll
	for (int k = 0; k < IT; k++) {
		const int i = threadIdx.x + k * GSR_LOSS_THREADS;
		const int r = i / GSR_LOSS_HX, q = i % GSR_LOSS_HX;
		const int gy = y0 + r, gx = x0 + q;
		const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
		if (i < N) {
			float x, y = yv[k];
			if constexpr (EXPO) x = gsr_expose(e, xv[0][k], xv[1][k], xv[2][k]);
			else x = xv[0][k];
			if constexpr (MASK) { x *= mv[k]; y *= mv[k]; }
			sx[r * GSR_LOSS_HXS + q] = in ? x : 0.f;
			sy[r * GSR_LOSS_HXS + q] = in ? y : 0.f;
		}
	}
}

template <bool MASK, bool EXPO, bool DEPTH>
__global__ void __launch_bounds__(GSR_LOSS_THREADS) gsr_ssim_ext_forward_kernel(const GsrLossExtForward a)
{
	__shared__ __attribute__((aligned(16))) float sx[GSR_LOSS_HY * GSR_LOSS_HXS], sy[GSR_LOSS_HY * GSR_LOSS_HXS];
	__shared__ __attribute__((aligned(16))) float tmp[5][GSR_LOSS_HY * GSR_LOSS_TX];
	__shared__ float wsum[GSR_LOSS_WAVES][3];
	static_assert(sizeof(sx) + sizeof(sy) + sizeof(tmp) + sizeof(wsum) <= 80 * 1024, "two workgroups per CU must fit gfx950's 160 KB of LDS");
	const int H = a.H, W = a.W;
	const int c = blockIdx.z;
	const size_t plane = (size_t)H * W;
	const int x0 = blockIdx.x * GSR_LOSS_TX - GSR_LOSS_R, y0 = blockIdx.y * GSR_LOSS_TY - GSR_LOSS_R;
	const GsrLossTaps& taps = a.taps;
	if constexpr (!MASK && !EXPO) {   // x'' = x, y'' = y: loss.hip's staging
		const float* const src[2] = {a.img + c * plane, a.gt + c * plane};
		float* const dst[2] = {sx, sy};
		gsr_loss_stage<2>(src, H, W, x0, y0, dst);
	} else {
		float e[4] = {1.f, 0.f, 0.f, 0.f};
		if constexpr (EXPO) gsr_exposure_column(a.exposure, c, e);
		gsr_loss_ext_stage<MASK, EXPO>(EXPO ? a.img : a.img + c * plane, a.gt + c * plane, a.mask, plane, e, H, W, x0, y0, sx, sy);
	}
	// this thread's own pixels (column lx, rows ly0..ly0+3) of the depth term are fetched now, used after both passes
	const int lx = threadIdx.x & 63, ly0 = (threadIdx.x >> 6) * 4;
	const int gx = blockIdx.x * GSR_LOSS_TX + lx;
	float dd[4] = {0.f, 0.f, 0.f, 0.f}, dk[4] = {0.f, 0.f, 0.f, 0.f};
	if (DEPTH && c == 0) {
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const int gy = blockIdx.y * GSR_LOSS_TY + ly0 + j;
			const size_t o = (gy < H && gx < W) ? (size_t)gy * W + gx : 0;
			dd[j] = a.invdepth[o] - a.prior[o];
			dk[j] = a.dmask ? a.dmask[o] : 1.f;
		}
	}
	__syncthreads();
	// horizontal pass: one row, four adjacent outputs of all five window means per work item;
	// x^2, y^2 and xy are formed in registers, never stored
	for (int it = threadIdx.x; it < GSR_LOSS_HY * GSR_LOSS_NQ; it += GSR_LOSS_THREADS) {
		const int r = it / GSR_LOSS_NQ, c4 = (it % GSR_LOSS_NQ) * 4;
		float xv[14], yv[14], pv[14];
		gsr_lds_load14(sx + r * GSR_LOSS_HXS + c4, xv);
		gsr_lds_load14(sy + r * GSR_LOSS_HXS + c4, yv);
		const int o = r * GSR_LOSS_TX + c4;
		*(float4*)(tmp[0] + o) = gsr_conv4(xv, taps);
		*(float4*)(tmp[1] + o) = gsr_conv4(yv, taps);
#pragma unroll
		for (int k = 0; k < 14; k++) pv[k] = xv[k] * xv[k];
		*(float4*)(tmp[2] + o) = gsr_conv4(pv, taps);
#pragma unroll
		for (int k = 0; k < 14; k++) pv[k] = yv[k] * yv[k];
		*(float4*)(tmp[3] + o) = gsr_conv4(pv, taps);
#pragma unroll
		for (int k = 0; k < 14; k++) pv[k] = xv[k] * yv[k];
		*(float4*)(tmp[4] + o) = gsr_conv4(pv, taps);
	}
	__syncthreads();

	// vertical pass + SSIM: column lx, four rows per thread (the per-pixel algebra is loss.hip's)
	const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
	const float4 m1 = gsr_conv_col4(tmp[0], ly0, lx, taps), m2 = gsr_conv_col4(tmp[1], ly0, lx, taps);
	const float4 q11 = gsr_conv_col4(tmp[2], ly0, lx, taps), q22 = gsr_conv_col4(tmp[3], ly0, lx, taps);
	const float4 q12 = gsr_conv_col4(tmp[4], ly0, lx, taps);
	const float mu1v[4] = {m1.x, m1.y, m1.z, m1.w}, mu2v[4] = {m2.x, m2.y, m2.z, m2.w};
	const float e11v[4] = {q11.x, q11.y, q11.z, q11.w}, e22v[4] = {q22.x, q22.y, q22.z, q22.w}, e12v[4] = {q12.x, q12.y, q12.z, q12.w};
	float l1 = 0.f, ss = 0.f, ld = 0.f;
#pragma unroll
	for (int j = 0; j < 4; j++) {
		const int ly = ly0 + j, gy = blockIdx.y * GSR_LOSS_TY + ly;
		if (gy >= H || gx >= W) continue;
		const float mu1 = mu1v[j], mu2 = mu2v[j], e11 = e11v[j], e22 = e22v[j], e12 = e12v[j];
		const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
		const float s11 = e11 - mu1_sq, s22 = e22 - mu2_sq, s12 = e12 - mu1_mu2;
		const float A1 = 2.f * mu1_mu2 + C1, A2 = 2.f * s12 + C2, B1 = mu1_sq + mu2_sq + C1, B2 = s11 + s22 + C2;
		const float inv = 1.f / (B1 * B2);
		const float S = (A1 * A2) * inv;
		const size_t op = (size_t)gy * W + gx, o = c * plane + op;
		a.dm[o] = (2.f * mu2 * (A2 - A1)) * inv - S * (2.f * mu1 * (B2 - B1)) * inv;
		a.d11[o] = -S / B2;
		a.d12[o] = 2.f * A1 * inv;
		ss += S;
		const int li = (ly + GSR_LOSS_R) * GSR_LOSS_HXS + lx + GSR_LOSS_R;
		l1 += fabsf(sx[li] - sy[li]);
		if (DEPTH && c == 0) {
			const float t = dd[j] * dk[j];
			ld += fabsf(t);
			if (a.dL_dinvdepth) {
				const float g = a.depth_scale * dk[j];
				a.dL_dinvdepth[op] = (t > 0.f) ? g : ((t < 0.f) ? -g : 0.f);
			}
		}
	}
	// fixed-order workgroup reduction -> one partial per tile (deterministic values)
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		l1 += __shfl_down(l1, off, 64);
		ss += __shfl_down(ss, off, 64);
		if constexpr (DEPTH) ld += __shfl_down(ld, off, 64);
	}
	if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6][0] = l1; wsum[threadIdx.x >> 6][1] = ss; wsum[threadIdx.x >> 6][2] = ld; }
	__syncthreads();
	if (threadIdx.x == 0) {
		float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
		for (int w = 0; w < GSR_LOSS_WAVES; w++) { t.x += wsum[w][0]; t.y += wsum[w][1]; t.z += wsum[w][2]; }
		a.partial[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = t;
	}
}

// gsr_loss_stage with the planes given from the image row `ry` (the first row this workgroup can touch) on, so that a lane's byte offset
// fits 32 bits and the load takes its base from scalar registers: the backward walks several channels, and 64-bit lane addresses
// kept across that loop did not fit its registers.
__device__ __forceinline__ const float* gsr_at(const float* base, unsigned bytes) { return (const float*)((const char*)base + bytes); }
__device__ __forceinline__ float* gsr_at(float* base, unsigned bytes) { return (float*)((char*)base + bytes); }

template <int NP>
__device__ __forceinline__ void gsr_loss_stage_rows(const float* const (&plane)[NP], int H, int W, int x0, int y0, int ry, int tid, float* const (&dst)[NP])
{
	constexpr int N = GSR_LOSS_HY * GSR_LOSS_HX, IT = (N + GSR_LOSS_THREADS - 1) / GSR_LOSS_THREADS;
	float v[NP][IT];
#pragma unroll
	for (int k = 0; k < IT; k++) {
		const int i = tid + k * GSR_LOSS_THREADS;
		const int r = i / GSR_LOSS_HX, q = i % GSR_LOSS_HX;
		const int gy = y0 + r, gx = x0 + q;
		const bool in = i < N && gy >= 0 && gy < H && gx >= 0 && gx < W;
		const unsigned o = in ? ((unsigned)(gy - ry) * (unsigned)W + (unsigned)gx) * 4u : 0u;   // in bytes
#pragma unroll
		for (int p = 0; p < NP; p++) { const float t = *gsr_at(plane[p], o); v[p][k] = in ? t : 0.f; }
	}
#pragma unroll
	for (int k = 0; k < IT; k++) {
		const int i = tid + k * GSR_LOSS_THREADS;
		const int r = i / GSR_LOSS_HX, q = i % GSR_LOSS_HX;
		if (i < N) {
#pragma unroll
			for (int p = 0; p < NP; p++) dst[p][r * GSR_LOSS_HXS + q] = v[p][k];
		}
	}
}

// Backward without exposure: loss.hip's kernel, one workgroup per tile and channel, with the mask at its two ends -- x'' and y'' of
// the own pixels, and G = m dloss/dx''.  The instantiation without a mask is that kernel instruction for instruction.
template <bool MASK>
__global__ void __launch_bounds__(GSR_LOSS_THREADS) gsr_ssim_ext_backward_kernel(int C, int H, int W, const float* __restrict__ img,
                                                                    const float* __restrict__ gt, const float* __restrict__ mask,
                                                                    GsrLossTaps taps, const float* __restrict__ dm,
                                                                    const float* __restrict__ d11, const float* __restrict__ d12,
                                                                    float lambda, float* __restrict__ dL_dimg)
{
	__shared__ __attribute__((aligned(16))) float s0[GSR_LOSS_HY * GSR_LOSS_HXS], s1[GSR_LOSS_HY * GSR_LOSS_HXS], s2[GSR_LOSS_HY * GSR_LOSS_HXS];
	__shared__ __attribute__((aligned(16))) float tmp[3][GSR_LOSS_HY * GSR_LOSS_TX];
	static_assert(sizeof(s0) * 3 + sizeof(tmp) <= 80 * 1024, "two workgroups per CU must fit gfx950's 160 KB of LDS");
	const int c = blockIdx.z;
	const size_t plane = (size_t)H * W;
	const int x0 = blockIdx.x * GSR_LOSS_TX - GSR_LOSS_R, y0 = blockIdx.y * GSR_LOSS_TY - GSR_LOSS_R;
	{
		const float* const src[3] = {dm + c * plane, d11 + c * plane, d12 + c * plane};
		float* const dst[3] = {s0, s1, s2};
		gsr_loss_stage<3>(src, H, W, x0, y0, dst);
	}
	// this thread's own pixels (column lx, rows ly0..ly0+3) are fetched now, used after both passes
	const int lx = threadIdx.x & 63, ly0 = (threadIdx.x >> 6) * 4;
	const int gx = blockIdx.x * GSR_LOSS_TX + lx;
	float xs[4], ys[4], ms[4];
#pragma unroll
	for (int j = 0; j < 4; j++) {
		const int gy = blockIdx.y * GSR_LOSS_TY + ly0 + j;
		const bool in = gy < H && gx < W;
		const size_t op = in ? (size_t)gy * W + gx : 0;
		const size_t o = in ? c * plane + (size_t)gy * W + gx : 0;
		xs[j] = img[o];
		ys[j] = gt[o];
		ms[j] = MASK ? mask[op] : 1.f;
	}
	__syncthreads();
	for (int it = threadIdx.x; it < GSR_LOSS_HY * GSR_LOSS_NQ; it += GSR_LOSS_THREADS) {
		const int r = it / GSR_LOSS_NQ, c4 = (it % GSR_LOSS_NQ) * 4;
		const int o = r * GSR_LOSS_TX + c4;
		float v[14];
		gsr_lds_load14(s0 + r * GSR_LOSS_HXS + c4, v);
		*(float4*)(tmp[0] + o) = gsr_conv4(v, taps);
		gsr_lds_load14(s1 + r * GSR_LOSS_HXS + c4, v);
		*(float4*)(tmp[1] + o) = gsr_conv4(v, taps);
		gsr_lds_load14(s2 + r * GSR_LOSS_HXS + c4, v);
		*(float4*)(tmp[2] + o) = gsr_conv4(v, taps);
	}
	__syncthreads();
	const float inv_total = 1.0f / ((float)C * (float)H * (float)W);
	const float4 a4 = gsr_conv_col4(tmp[0], ly0, lx, taps), b4 = gsr_conv_col4(tmp[1], ly0, lx, taps), c4v = gsr_conv_col4(tmp[2], ly0, lx, taps);
	const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w}, cv[4] = {c4v.x, c4v.y, c4v.z, c4v.w};
#pragma unroll
	for (int j = 0; j < 4; j++) {
		const int gy = blockIdx.y * GSR_LOSS_TY + ly0 + j;
		if (gy >= H || gx >= W) continue;
		const size_t o = c * plane + (size_t)gy * W + gx;
		float xv = xs[j], yv = ys[j];
		if constexpr (MASK) { xv *= ms[j]; yv *= ms[j]; }
		const float dssim = av[j] + 2.f * xv * bv[j] + yv * cv[j];
		const float sgn = (xv > yv) ? 1.f : ((xv < yv) ? -1.f : 0.f);
		float g = ((1.f - lambda) * sgn - lambda * dssim) * inv_total;   // dloss/dx''
		if constexpr (MASK) g = (ms[j] == 0.f) ? 0.f : ms[j] * g;        // +0.0 where the mask is 0: the window term there is not
		dL_dimg[o] = g;
	}
}

// Backward with exposure: dL/dimg_k = sum_c E[k][c] G_c needs all three G_c, so one workgroup walks the three channels of its tile.
// (Second launch bound: four waves per SIMD, i.e. at most 128 VGPRs -- the two resident workgroups the LDS allows; without it the
// kernel took 146-152.)
template <bool MASK>
__global__ void __launch_bounds__(GSR_LOSS_THREADS, 4) gsr_ssim_ext_backward_exposure_kernel(const GsrLossExtBackward a)
{
	__shared__ __attribute__((aligned(16))) float s0[GSR_LOSS_HY * GSR_LOSS_HXS], s1[GSR_LOSS_HY * GSR_LOSS_HXS], s2[GSR_LOSS_HY * GSR_LOSS_HXS];
	__shared__ __attribute__((aligned(16))) float tmp[3][GSR_LOSS_HY * GSR_LOSS_TX];
	__shared__ float wsum[GSR_LOSS_WAVES][12];
	static_assert(sizeof(s0) * 3 + sizeof(tmp) + sizeof(wsum) <= 80 * 1024, "two workgroups per CU must fit gfx950's 160 KB of LDS");
	const int H = a.H, W = a.W;
	const size_t plane = (size_t)H * W;
	const int x0 = blockIdx.x * GSR_LOSS_TX - GSR_LOSS_R, y0 = blockIdx.y * GSR_LOSS_TY - GSR_LOSS_R;
	const GsrLossTaps& taps = a.taps;
	// A thread's own pixels are column lx, rows ly0..ly0+3.  dL/dimg of the three channels stays in registers; the raw planes and the
	// mask are fetched again for every channel (cache hits) rather than held across the passes.  Offsets count in bytes from image
	// row ry on (gsr_loss_stage_rows): 32 bits per lane beside a scalar base.
	const int ry = y0 > 0 ? y0 : 0;
	const size_t row0 = (size_t)ry * W;
	float acc[3][4];
#pragma unroll
	for (int j = 0; j < 4; j++) {
#pragma unroll
		for (int p = 0; p < 3; p++) acc[p][j] = 0.f;
	}
	const float inv_total = 1.0f / (3.f * (float)H * (float)W);
#pragma unroll 1
	for (int c = 0; c < 3; c++) {
		// Everything that depends on the thread alone (staging offsets, LDS addresses, the own pixels' offsets) is invariant in this
		// loop; hoisted out of it, it took ~50 registers more than there are and came back as spills that the staging loads then
		// waited for one by one.  An id the compiler cannot see through makes every channel recompute it.
		int tid = threadIdx.x;
		asm volatile("" : "+v"(tid));
		const int lx = tid & 63, ly0 = (tid >> 6) * 4;
		const int gx = blockIdx.x * GSR_LOSS_TX + lx;
		unsigned po[4];
		bool in[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const int gy = blockIdx.y * GSR_LOSS_TY + ly0 + j;
			in[j] = gy < H && gx < W;
			po[j] = in[j] ? ((unsigned)(gy - ry) * (unsigned)W + (unsigned)gx) * 4u : 0u;
		}
		{
			const float* const src[3] = {a.dm + c * plane + row0, a.d11 + c * plane + row0, a.d12 + c * plane + row0};
			float* const dst[3] = {s0, s1, s2};
			gsr_loss_stage_rows<3>(src, H, W, x0, y0, ry, tid, dst);   // the previous channel's reads of s0..s2 ended before its second barrier
		}
		__syncthreads();   // also: every thread is past the previous channel's reads of tmp
		for (int it = tid; it < GSR_LOSS_HY * GSR_LOSS_NQ; it += GSR_LOSS_THREADS) {
			const int r = it / GSR_LOSS_NQ, c4 = (it % GSR_LOSS_NQ) * 4;
			const int o = r * GSR_LOSS_TX + c4;
			float v[14];
			gsr_lds_load14(s0 + r * GSR_LOSS_HXS + c4, v);
			*(float4*)(tmp[0] + o) = gsr_conv4(v, taps);
			gsr_lds_load14(s1 + r * GSR_LOSS_HXS + c4, v);
			*(float4*)(tmp[1] + o) = gsr_conv4(v, taps);
			gsr_lds_load14(s2 + r * GSR_LOSS_HXS + c4, v);
			*(float4*)(tmp[2] + o) = gsr_conv4(v, taps);
		}
		// the own pixels' inputs are fetched after the horizontal pass, which has no registers to spare for them, and used after the
		// vertical one
		float xr[3][4], ys[4], mk[4], e[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
#pragma unroll
			for (int p = 0; p < 3; p++) xr[p][j] = *gsr_at(a.img + p * plane + row0, po[j]);
			ys[j] = *gsr_at(a.gt + c * plane + row0, po[j]);
			mk[j] = MASK ? *gsr_at(a.mask + row0, po[j]) : 1.f;
		}
		gsr_exposure_column(a.exposure, c, e);
		__syncthreads();
		const float4 a4 = gsr_conv_col4(tmp[0], ly0, lx, taps), b4 = gsr_conv_col4(tmp[1], ly0, lx, taps), c4v = gsr_conv_col4(tmp[2], ly0, lx, taps);
		const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w}, cv[4] = {c4v.x, c4v.y, c4v.z, c4v.w};
		float ex[4] = {0.f, 0.f, 0.f, 0.f};   // sums of G_c x_0, G_c x_1, G_c x_2, G_c over this thread's pixels
#pragma unroll
		for (int j = 0; j < 4; j++) {
			if (!in[j]) continue;
			float xv = gsr_expose(e, xr[0][j], xr[1][j], xr[2][j]), yv = ys[j];
			if constexpr (MASK) { xv *= mk[j]; yv *= mk[j]; }
			const float dssim = av[j] + 2.f * xv * bv[j] + yv * cv[j];
			const float sgn = (xv > yv) ? 1.f : ((xv < yv) ? -1.f : 0.f);
			float g = ((1.f - a.lambda) * sgn - a.lambda * dssim) * inv_total;   // dloss/dx''_c
			if constexpr (MASK) g = (mk[j] == 0.f) ? 0.f : mk[j] * g;            // G_c; +0.0 where the mask is 0
#pragma unroll
			for (int k = 0; k < 3; k++) {
				acc[k][j] = __builtin_fmaf(e[k], g, acc[k][j]);
				ex[k] = __builtin_fmaf(g, xr[k][j], ex[k]);
			}
			ex[3] += g;
		}
		if (a.epart) {   // wave sums now, the workgroup's after the last channel: the slots of the three channels are disjoint
#pragma unroll
			for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
				for (int k = 0; k < 4; k++) ex[k] += __shfl_down(ex[k], off, 64);
			}
			if (lx == 0) {
#pragma unroll
				for (int k = 0; k < 3; k++) wsum[tid >> 6][4 * k + c] = ex[k];
				wsum[tid >> 6][4 * c + 3] = ex[3];
			}
		}
	}
	if (a.dL_dimg) {
		const int lx = threadIdx.x & 63, ly0 = (threadIdx.x >> 6) * 4;
		const int gx = blockIdx.x * GSR_LOSS_TX + lx;
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const int gy = blockIdx.y * GSR_LOSS_TY + ly0 + j;
			if (gy >= H || gx >= W) continue;
			const unsigned o = ((unsigned)(gy - ry) * (unsigned)W + (unsigned)gx) * 4u;
#pragma unroll
			for (int p = 0; p < 3; p++) *gsr_at(a.dL_dimg + p * plane + row0, o) = acc[p][j];
		}
	}
	if (a.epart) {
		__syncthreads();
		if (threadIdx.x < 12) {
			float t = 0.f;
#pragma unroll
			for (int w = 0; w < GSR_LOSS_WAVES; w++) t += wsum[w][threadIdx.x];
			a.epart[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 12 + threadIdx.x] = t;
		}
	}
}

// One workgroup folds the per-tile sums in a fixed order in double: vals = {loss, l1, ssim, depth_l1} and, with EXPO, the twelve
// entries of dL_dexposure from the backward's per-tile sums (without it the fold carries three sums, not fifteen).
template <bool EXPO>
__global__ void __launch_bounds__(256) gsr_loss_ext_finalize_kernel(const float4* __restrict__ partial, int n, const float* __restrict__ epart,
                                                                    int ne, int C, int H, int W, float lambda, float weight,
                                                                    float* __restrict__ vals, float* __restrict__ dL_dexposure)
{
	constexpr int NQ = EXPO ? 15 : 3;
	__shared__ double sw[4][NQ];
	double v[NQ];
#pragma unroll
	for (int q = 0; q < NQ; q++) v[q] = 0.0;
	for (int i = threadIdx.x; i < n; i += 256) { const float4 p = partial[i]; v[0] += p.x; v[1] += p.y; v[2] += p.z; }
	if constexpr (EXPO) {
		for (int i = threadIdx.x; i < ne; i += 256) {
#pragma unroll
			for (int q = 0; q < 12; q++) v[3 + q] += epart[(size_t)i * 12 + q];
		}
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
		for (int q = 0; q < NQ; q++) v[q] += __shfl_down(v[q], off, 64);
	}
	if ((threadIdx.x & 63) == 0) {
#pragma unroll
		for (int q = 0; q < NQ; q++) sw[threadIdx.x >> 6][q] = v[q];
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		const double total = (double)C * H * W, pixels = (double)H * W;
		const double ml1 = (sw[0][0] + sw[1][0] + sw[2][0] + sw[3][0]) / total, mss = (sw[0][1] + sw[1][1] + sw[2][1] + sw[3][1]) / total;
		const double mld = (sw[0][2] + sw[1][2] + sw[2][2] + sw[3][2]) / pixels;
		vals[0] = (float)((1.0 - lambda) * ml1 + lambda * (1.0 - mss) + (double)weight * mld);
		vals[1] = (float)ml1;
		vals[2] = (float)mss;
		vals[3] = (float)mld;
	}
	if constexpr (EXPO) {
		if (threadIdx.x < 12) {
			const int q = 3 + threadIdx.x;
			dL_dexposure[threadIdx.x] = (float)(sw[0][q] + sw[1][q] + sw[2][q] + sw[3][q]);
		}
	}
}

size_t gsr_loss_ext_scratch_layout(int C, int H, int W, size_t* maps_off, size_t* partial_off, size_t* epart_off, int* ntiles, int* ntiles_xy)
{
	const size_t n = (size_t)C * H * W;
	const int gx = (W + GSR_LOSS_TX - 1) / GSR_LOSS_TX, gy = (H + GSR_LOSS_TY - 1) / GSR_LOSS_TY;
	*ntiles_xy = gx * gy;
	*ntiles = gx * gy * C;
	*maps_off = 0;
	*partial_off = gsr_align_up(3 * n * sizeof(float));
	*epart_off = *partial_off + gsr_align_up((size_t)(*ntiles) * sizeof(float4));
	return *epart_off + gsr_align_up((size_t)(*ntiles_xy) * 12 * sizeof(float));
}

template <bool MASK, bool EXPO>
static void gsr_launch_ext_forward(bool depth, dim3 grid, hipStream_t s, const GsrLossExtForward& f)
{
	if (depth) hipLaunchKernelGGL((gsr_ssim_ext_forward_kernel<MASK, EXPO, true>), grid, dim3(GSR_LOSS_THREADS), 0, s, f);
	else hipLaunchKernelGGL((gsr_ssim_ext_forward_kernel<MASK, EXPO, false>), grid, dim3(GSR_LOSS_THREADS), 0, s, f);
}

void gsr_launch_l1_ssim_ext(const gsr_loss_ext_args& a, hipStream_t s)
{
	const int C = a.C, H = a.H, W = a.W;
	size_t maps_off, partial_off, epart_off;
	int ntiles, ntiles_xy;
	gsr_loss_ext_scratch_layout(C, H, W, &maps_off, &partial_off, &epart_off, &ntiles, &ntiles_xy);
	const size_t n = (size_t)C * H * W;
	float* dm = (float*)((char*)a.scratch + maps_off);
	float* d11 = dm + n;
	float* d12 = d11 + n;
	float4* partial = (float4*)((char*)a.scratch + partial_off);
	float* epart = (float*)((char*)a.scratch + epart_off);
	const bool mask = a.mask != nullptr, expo = a.exposure != nullptr, depth = a.invdepth != nullptr;
	const bool want_expo = expo && a.dL_dexposure;
	const dim3 grid((W + GSR_LOSS_TX - 1) / GSR_LOSS_TX, (H + GSR_LOSS_TY - 1) / GSR_LOSS_TY, C);
	{
		GsrProfScope p(s, "ssim_ext_forward");
		GsrLossExtForward f;
		f.H = H; f.W = W;
		f.img = a.img; f.gt = a.gt; f.mask = a.mask; f.exposure = a.exposure;
		f.invdepth = a.invdepth; f.prior = a.invdepth_prior; f.dmask = a.invdepth_mask;
		f.depth_scale = (float)((double)a.invdepth_weight / ((double)H * W));
		f.taps = gsr_loss_taps();
		f.dm = dm; f.d11 = d11; f.d12 = d12; f.dL_dinvdepth = a.dL_dinvdepth;
		f.partial = partial;
		if (mask && expo) gsr_launch_ext_forward<true, true>(depth, grid, s, f);
		else if (mask) gsr_launch_ext_forward<true, false>(depth, grid, s, f);
		else if (expo) gsr_launch_ext_forward<false, true>(depth, grid, s, f);
		else gsr_launch_ext_forward<false, false>(depth, grid, s, f);
	}
	if (expo && (a.dL_dimg || want_expo)) {
		GsrProfScope p(s, "ssim_ext_backward");
		GsrLossExtBackward b;
		b.H = H; b.W = W;
		b.img = a.img; b.gt = a.gt; b.mask = a.mask; b.exposure = a.exposure;
		b.taps = gsr_loss_taps();
		b.dm = dm; b.d11 = d11; b.d12 = d12;
		b.lambda = a.lambda_dssim;
		b.dL_dimg = a.dL_dimg;
		b.epart = want_expo ? epart : nullptr;
		const dim3 bgrid(grid.x, grid.y, 1), block(GSR_LOSS_THREADS);
		if (mask) hipLaunchKernelGGL(gsr_ssim_ext_backward_exposure_kernel<true>, bgrid, block, 0, s, b);
		else hipLaunchKernelGGL(gsr_ssim_ext_backward_exposure_kernel<false>, bgrid, block, 0, s, b);
	} else if (a.dL_dimg) {
		GsrProfScope p(s, "ssim_ext_backward");
		const GsrLossTaps taps = gsr_loss_taps();
		const dim3 block(GSR_LOSS_THREADS);
		if (mask) hipLaunchKernelGGL(gsr_ssim_ext_backward_kernel<true>, grid, block, 0, s, C, H, W, a.img, a.gt, a.mask, taps, dm, d11, d12, a.lambda_dssim, a.dL_dimg);
		else hipLaunchKernelGGL(gsr_ssim_ext_backward_kernel<false>, grid, block, 0, s, C, H, W, a.img, a.gt, a.mask, taps, dm, d11, d12, a.lambda_dssim, a.dL_dimg);
	}
	const float weight = depth ? a.invdepth_weight : 0.f;
	if (want_expo)
		hipLaunchKernelGGL(gsr_loss_ext_finalize_kernel<true>, dim3(1), dim3(256), 0, s, partial, ntiles, epart, ntiles_xy, C, H, W,
		                   a.lambda_dssim, weight, a.vals, a.dL_dexposure);
	else
		hipLaunchKernelGGL(gsr_loss_ext_finalize_kernel<false>, dim3(1), dim3(256), 0, s, partial, ntiles, epart, 0, C, H, W,
		                   a.lambda_dssim, weight, a.vals, a.dL_dexposure);
}
