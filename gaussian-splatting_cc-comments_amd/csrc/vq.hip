// vq.hip -- vector quantisation: nearest-code search on the fp32-input matrix cores and the fixed-order centroid update
// (include/gsr_vq.h; compiled with -ffp-contract=off, every fma outside the MFMA is written out).
//
// assign.  v_mfma_f32_32x32x2_f32 computes D[i][j] = fmaf(A[i][1], B[1][j], fmaf(A[i][0], B[0][j], C[i][j])): a k-ordered fp32 fmaf
// chain, which is the score the header specifies.  Codes are the rows i (operand A), data rows the columns j (operand B = -2 x), c2
// the C input.  Lane l holds A[l & 31][l >> 5] and B[l >> 5][l & 31]; of the result it holds column l & 31 and the rows
// (r & 3) + 8 (r >> 2) + 4 (l >> 5), r = 0 .. 15: one data row per lane, sixteen codes in its accumulator, ascending in r.
//   * A workgroup is four waves and 256 data rows; a wave keeps its 64 rows (two column tiles) as B operands in registers for the
//     whole launch: 2 KS registers, KS = the number of k steps of two.
//   * A pre-pass writes c2 and the codebook transposed, [tile of 128 codes][k][code], zero-padded in k and in the last tile, whose
//     missing codes get c2 = +inf and never win.  A tile is then one straight 16-byte copy into the LDS; a row of the image is 160
//     floats, so that the two lane halves of an operand read (rows k and k + 1) fall on different halves of the 64 banks.
//   * Per 64 codes a wave issues 4 KS MFMAs into four independent accumulators (2 code tiles x 2 column tiles, two LDS reads per
//     four MFMAs), then compares the 64 scores on the VALU.  A lane meets its codes in ascending index order and replaces on `<`
//     only; the two halves of a column are combined at the end with the index as the tie break.  Data rows are not shared between
//     waves, so there is no further combine.
//   * dist2 is evaluated at the end, by the lane that owns the row, in double.
// Registers: 64 accumulators + up to 64 operands + 4 for the running best; LDS: (2 KS * 160 + 128) floats, 41.5 KB at D = 64.
//
// update.  A workgroup per code, lane d of a wave owns column d and walks its part of the member list in order with the rows read
// coalesced; sixteen members' loads are in flight while the sixteen before them are added one by one.  Lists of 512 members and more
// are cut into up to sixteen parts by their length alone (below).
#include "gsr_internal.h"
#include "gsr_depth_key.h"
#include "../../include/gsr_vq.h"

#include <math.h>

#define GSR_VQ_TILE 128                         // codes per LDS tile
#define GSR_VQ_STRIDE (GSR_VQ_TILE + 32)        // floats per k row of the LDS image
#define GSR_VQ_ROWS 256                         // data rows per workgroup (4 waves x 64)

typedef float gsr_f32x16 __attribute__((ext_vector_type(16)));

// k steps of two the kernel is instantiated for: the smallest that holds D
static int gsr_vq_ksteps(int D) { return D <= 8 ? 4 : D <= 16 ? 8 : D <= 32 ? 16 : D <= 48 ? 24 : 32; }
static int gsr_vq_tiles(int K) { return (K + GSR_VQ_TILE - 1) / GSR_VQ_TILE; }

// c2 [tiles * 128] and the transposed image ct [tiles][DK][128]; a thread per padded code
__global__ void __launch_bounds__(256) gsr_vq_prepare_kernel(int K, int D, int DK, int padded, const float* __restrict__ codebook, float* __restrict__ c2,
                                                             float* __restrict__ ct)
{
	const int j = blockIdx.x * 256 + threadIdx.x;
	if (j >= padded) return;
	float* out = ct + (size_t)(j / GSR_VQ_TILE) * (size_t)DK * GSR_VQ_TILE + (j % GSR_VQ_TILE);
	float acc = 0.f;
	for (int k = 0; k < DK; k++) {
		const float c = (j < K && k < D) ? codebook[(size_t)j * D + k] : 0.f;
		acc = __builtin_fmaf(c, c, acc);   // the padding adds fmaf(0, 0, acc) = acc
		out[(size_t)k * GSR_VQ_TILE] = c;
	}
	c2[j] = j < K ? acc : INFINITY;
}

// the sixteen scores of one accumulator against the lane's running best; code = the index of register 0's code
__device__ __forceinline__ void gsr_vq_take(const gsr_f32x16& acc, int code, float& best, int& arg)
{
#pragma unroll
	for (int r = 0; r < 16; r++) {
		const bool less = acc[r] < best;
		best = less ? acc[r] : best;
		arg = less ? code + (r & 3) + 8 * (r >> 2) : arg;
	}
}

// the other half's best of the same column: smaller score, or the same score and a smaller index
__device__ __forceinline__ void gsr_vq_merge_halves(float& best, int& arg)
{
	const float ob = __shfl_xor(best, 32, 64);
	const int oa = __shfl_xor(arg, 32, 64);
	const bool take = ob < best || (ob == best && oa < arg);
	best = take ? ob : best;
	arg = take ? oa : arg;
}

template <int KS>
__global__ void __launch_bounds__(256) gsr_vq_assign_kernel(int N, int D, int K, int tiles, const float* __restrict__ x, const float* __restrict__ codebook,
                                                            const float* __restrict__ c2, const float* __restrict__ ct, int* __restrict__ idx,
                                                            float* __restrict__ dist2)
{
	constexpr int DK = 2 * KS;
	__shared__ __attribute__((aligned(16))) float image[DK * GSR_VQ_STRIDE];
	__shared__ __attribute__((aligned(16))) float c2s[GSR_VQ_TILE];
	const int lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
	const long long base = (long long)blockIdx.x * GSR_VQ_ROWS + (threadIdx.x >> 6) * 64;
	const long long row0 = base + col, row1 = base + 32 + col;

	// the wave's rows as B operands: lane (col, half) holds -2 x[row][2 s + half]
	float b0[KS], b1[KS];
#pragma unroll
	for (int s = 0; s < KS; s++) {
		const int k = 2 * s + half;
		b0[s] = (row0 < N && k < D) ? -2.f * x[(size_t)row0 * D + k] : 0.f;
		b1[s] = (row1 < N && k < D) ? -2.f * x[(size_t)row1 * D + k] : 0.f;
	}
	float best0 = INFINITY, best1 = INFINITY;
	int arg0 = -1, arg1 = -1;

	for (int t = 0; t < tiles; t++) {
		gsr_sync();   // the tile before has been read by every wave
		const float4* src = (const float4*)(ct + (size_t)t * DK * GSR_VQ_TILE);
		for (int e = threadIdx.x; e < DK * (GSR_VQ_TILE / 4); e += 256) {
			const int k = e / (GSR_VQ_TILE / 4), c4 = e % (GSR_VQ_TILE / 4);
			*(float4*)(image + k * GSR_VQ_STRIDE + 4 * c4) = src[e];
		}
		if (threadIdx.x < GSR_VQ_TILE) c2s[threadIdx.x] = c2[t * GSR_VQ_TILE + threadIdx.x];
		gsr_sync();
#pragma unroll 1
		for (int sub = 0; sub < GSR_VQ_TILE; sub += 64) {
			gsr_f32x16 acc00, acc01, acc10, acc11;   // acc<code tile><column tile>
#pragma unroll
			for (int r = 0; r < 16; r++) {
				const int i = (r & 3) + 8 * (r >> 2) + 4 * half;
				const float lo = c2s[sub + i], hi = c2s[sub + 32 + i];
				acc00[r] = lo; acc01[r] = lo; acc10[r] = hi; acc11[r] = hi;
			}
#pragma unroll
			for (int s = 0; s < KS; s++) {
				const float a0 = image[(2 * s + half) * GSR_VQ_STRIDE + sub + col];
				const float a1 = image[(2 * s + half) * GSR_VQ_STRIDE + sub + 32 + col];
				acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0[s], acc00, 0, 0, 0);
				acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1[s], acc01, 0, 0, 0);
				acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0[s], acc10, 0, 0, 0);
				acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1[s], acc11, 0, 0, 0);
			}
			const int code = t * GSR_VQ_TILE + sub + 4 * half;   // ascending within the lane: tile, sub, code tile, register
			gsr_vq_take(acc00, code, best0, arg0);
			gsr_vq_take(acc10, code + 32, best0, arg0);
			gsr_vq_take(acc01, code, best1, arg1);
			gsr_vq_take(acc11, code + 32, best1, arg1);
		}
	}
	gsr_vq_merge_halves(best0, arg0);
	gsr_vq_merge_halves(best1, arg1);

	// the lower half writes column tile 0, the upper half column tile 1
	const long long row = half ? row1 : row0;
	const int j = half ? arg1 : arg0;
	if (row >= N) return;
	idx[row] = j;
	if (dist2) {
		float out = NAN;
		if (j >= 0) {
			double acc = 0.0;
			for (int k = 0; k < D; k++) {
				const double d = (double)x[(size_t)row * D + k] - (double)codebook[(size_t)j * D + k];
				acc = __builtin_fma(d, d, acc);
			}
			out = (float)acc;
		}
		dist2[row] = out;
	}
}

size_t gsr_vq_assign_scratch_size(int N, int D, int K)
{
	if (N < 0 || D < 1 || D > GSR_VQ_MAX_D || K < 1 || K > GSR_VQ_MAX_K) return 0;
	const size_t padded = (size_t)gsr_vq_tiles(K) * GSR_VQ_TILE;
	return gsr_align_up(4 * padded) + gsr_align_up(4 * padded * 2 * (size_t)gsr_vq_ksteps(D));
}

template <int KS>
static void gsr_vq_assign_launch(int N, int D, int K, const float* x, const float* codebook, const float* c2, const float* ct, int* idx, float* dist2,
                                 hipStream_t s)
{
	hipLaunchKernelGGL(gsr_vq_assign_kernel<KS>, dim3((unsigned)(((long long)N + GSR_VQ_ROWS - 1) / GSR_VQ_ROWS)), dim3(256), 0, s, N, D, K, gsr_vq_tiles(K), x,
	                   codebook, c2, ct, idx, dist2);
}

void gsr_launch_vq_assign(int N, int D, const float* x, int K, const float* codebook, int* idx, float* dist2, void* scratch, hipStream_t s)
{
	GsrProfScope p(s, "vq_assign");
	const int KS = gsr_vq_ksteps(D), padded = gsr_vq_tiles(K) * GSR_VQ_TILE;
	float* c2 = (float*)scratch;
	float* ct = (float*)((char*)scratch + gsr_align_up(4 * (size_t)padded));
	hipLaunchKernelGGL(gsr_vq_prepare_kernel, dim3(padded / 256 + 1), dim3(256), 0, s, K, D, 2 * KS, padded, codebook, c2, ct);
	switch (KS) {
	case 4: gsr_vq_assign_launch<4>(N, D, K, x, codebook, c2, ct, idx, dist2, s); break;
	case 8: gsr_vq_assign_launch<8>(N, D, K, x, codebook, c2, ct, idx, dist2, s); break;
	case 16: gsr_vq_assign_launch<16>(N, D, K, x, codebook, c2, ct, idx, dist2, s); break;
	case 24: gsr_vq_assign_launch<24>(N, D, K, x, codebook, c2, ct, idx, dist2, s); break;
	default: gsr_vq_assign_launch<32>(N, D, K, x, codebook, c2, ct, idx, dist2, s); break;
	}
}

// ---- update ----
// A workgroup of sixteen waves per code.  A list of L members is cut into P = min(16, max(1, L / 256)) parts of Q = ceil(L / P)
// members (the last one shorter): a function of L alone.  Wave p adds part p one member after the other from +0; wave 0 then adds
// the parts' sums in ascending part order.  Below 512 members that is the plain sequential sum by one wave.
#define GSR_VQ_BATCH 16
#define GSR_VQ_PARTS 16
#define GSR_VQ_PART_MIN 256
__global__ void __launch_bounds__(64 * GSR_VQ_PARTS) gsr_vq_update_kernel(int D, int K, const float* __restrict__ x, const float* __restrict__ weight,
                                                                          const int* __restrict__ offsets, const int* __restrict__ members,
                                                                          float* __restrict__ codebook, int* __restrict__ count, float* __restrict__ wsum)
{
	__shared__ double part_s[GSR_VQ_PARTS][64];
	__shared__ double part_w[GSR_VQ_PARTS];
	const int j = blockIdx.x, p = threadIdx.x >> 6, d = threadIdx.x & 63;
	const int lo = offsets[j], hi = offsets[j + 1], L = hi - lo;
	const int P = min(GSR_VQ_PARTS, max(1, L / GSR_VQ_PART_MIN)), Q = (L + P - 1) / P;   // uniform over the workgroup
	if (P == 1 && p > 0) return;
	const int dd = d < D ? d : D - 1;   // lanes past the last column repeat it and write nothing
	double S = 0.0, W = 0.0;
	if (p < P) {
		int m = min(hi, lo + p * Q);
		const int end = min(hi, m + Q);
		for (; m + GSR_VQ_BATCH <= end; m += GSR_VQ_BATCH) {
			float v[GSR_VQ_BATCH], w[GSR_VQ_BATCH];
#pragma unroll
			for (int b = 0; b < GSR_VQ_BATCH; b++) {
				const int i = members[m + b];
				v[b] = x[(size_t)i * D + dd];
				w[b] = weight ? weight[i] : 1.f;
			}
#pragma unroll
			for (int b = 0; b < GSR_VQ_BATCH; b++) {
				S = S + (double)w[b] * (double)v[b];   // the product is exact in double
				W = W + (double)w[b];
			}
		}
		for (; m < end; m++) {
			const int i = members[m];
			const double w = weight ? (double)weight[i] : 1.0;
			S = S + w * (double)x[(size_t)i * D + dd];
			W = W + w;
		}
	}
	if (P > 1) {
		part_s[p][d] = S;
		if (d == 0) part_w[p] = W;
		gsr_sync();
		if (p > 0) return;
		for (int q = 1; q < P; q++) {
			S = S + part_s[q][d];
			W = W + part_w[q];
		}
	}
	if (d == 0) {
		if (count) count[j] = L;
		if (wsum) wsum[j] = (float)W;
	}
	if (d < D && L > 0 && W != 0.0) codebook[(size_t)j * D + d] = (float)(S / W);
}

void gsr_launch_vq_update(int D, const float* x, const float* weight, int K, const int* offsets, const int* members, float* codebook, int* count,
                          float* wsum, hipStream_t s)
{
	GsrProfScope p(s, "vq_update");
	hipLaunchKernelGGL(gsr_vq_update_kernel, dim3(K), dim3(64 * GSR_VQ_PARTS), 0, s, D, K, x, weight, offsets, members, codebook, count, wsum);
}
