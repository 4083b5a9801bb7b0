// gsr_loss_tile.h -- the tile geometry and the separable 11-tap window passes that the fused losses share (loss.hip, loss_ext.hip).
#pragma once
#include "gsr_internal.h"

#define GSR_LOSS_TX 64
// tile height: 16 / 32 rows -> 0.151 / 0.137 ms for the 1980x1080 loss (fwd + bwd), 0.59 / 0.52 ms at 3840x2160: the taller tile
// re-reads less halo (42 / 32 rows instead of 26 / 16) and its 512-thread workgroups fill the SIMDs better
// 32-row tiles need ~79 KB (forward) / ~70 KB (backward) of static LDS per workgroup: more than the 64 KB of every gfx9
// part except gfx950 (160 KB per CU, two workgroups resident).  This library is built for gfx950 only (csrc/Makefile);
// -DGSR_LOSS_TY=16 is the variant that fits 64 KB, should the ARCH override of the Makefile ever be used.
#ifndef GSR_LOSS_TY
#define GSR_LOSS_TY 32
#endif
#define GSR_LOSS_THREADS (64 * (GSR_LOSS_TY / 4))  // one column and four rows of the tile per thread in the vertical pass
#define GSR_LOSS_R 5
#define GSR_LOSS_HX (GSR_LOSS_TX + 2 * GSR_LOSS_R)  // 74 columns with halo
#define GSR_LOSS_HXS 76                               // row stride in LDS: multiple of 4 floats so b128 reads stay aligned
#define GSR_LOSS_HY (GSR_LOSS_TY + 2 * GSR_LOSS_R)  // 42 rows with halo
#define GSR_LOSS_NQ (GSR_LOSS_TX / 4)                 // quads of outputs per row

struct GsrLossTaps { float g[11]; };

// 14 consecutive floats starting at a 16-byte aligned LDS address
__device__ __forceinline__ void gsr_lds_load14(const float* __restrict__ p, float (&v)[14])
{
	const float4 a = ((const float4*)p)[0], b = ((const float4*)p)[1], c = ((const float4*)p)[2];
	const float2 d = ((const float2*)p)[6];
	v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
	v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w; v[12] = d.x; v[13] = d.y;
}

// four adjacent outputs of the 11-tap window over 14 inputs held in registers (taps in ascending order)
__device__ __forceinline__ float4 gsr_conv4(const float (&v)[14], const GsrLossTaps& t)
{
	float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
	for (int k = 0; k < 11; k++) {
#pragma unroll
		for (int j = 0; j < 4; j++) o[j] += t.g[k] * v[j + k];
	}
	return make_float4(o[0], o[1], o[2], o[3]);
}

// zero-padded (F.conv2d padding=5) tile + halo of NP planes -> LDS [HY][HXS] each.  All global loads
// of a thread are issued before the first LDS store, so one round of memory latency covers them.
template <int NP>
__device__ __forceinline__ void gsr_loss_stage(const float* const (&plane)[NP], int H, int W, int x0, int y0, float* const (&dst)[NP])
{
	constexpr int N = GSR_LOSS_HY * GSR_LOSS_HX, IT = (N + GSR_LOSS_THREADS - 1) / GSR_LOSS_THREADS;
	float v[NP][IT];
#pragma unroll
	for (int k = 0; k < IT; k++) {
		const int i = threadIdx.x + k * GSR_LOSS_THREADS;
		const int r = i / GSR_LOSS_HX, q = i % GSR_LOSS_HX;
		const int gy = y0 + r, gx = x0 + q;
		const bool in = i < N && gy >= 0 && gy < H && gx >= 0 && gx < W;
		const size_t o = in ? (size_t)gy * W + gx : 0;
#pragma unroll
		for (int p = 0; p < NP; p++) { const float t = plane[p][o]; v[p][k] = in ? t : 0.f; }
	}
#pragma unroll
	for (int k = 0; k < IT; k++) {
		const int i = threadIdx.x + k * GSR_LOSS_THREADS;
		const int r = i / GSR_LOSS_HX, q = i % GSR_LOSS_HX;
		if (i < N) {
#pragma unroll
			for (int p = 0; p < NP; p++) dst[p][r * GSR_LOSS_HXS + q] = v[p][k];
		}
	}
}

// vertical pass: this thread's column lx, output rows ly0..ly0+3, from a row-filtered plane [HY][TX]
__device__ __forceinline__ float4 gsr_conv_col4(const float* __restrict__ tmp, int ly0, int lx, const GsrLossTaps& t)
{
	float v[14];
#pragma unroll
	for (int k = 0; k < 14; k++) v[k] = tmp[(ly0 + k) * GSR_LOSS_TX + lx];
	return gsr_conv4(v, t);
}

static inline GsrLossTaps gsr_loss_taps()
{
	// loss_utils.py:21-24: float32 tensor of exp(-(x-5)^2 / (2 sigma^2)), divided by its float32 sum
	GsrLossTaps t;
	float raw[11], sum = 0.f;
	for (int i = 0; i < 11; i++) raw[i] = (float)exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
	for (int i = 0; i < 11; i++) sum += raw[i];
	for (int i = 0; i < 11; i++) t.g[i] = raw[i] / sum;
	return t;
}
