// densify.hip -- clone, split and prune as one compaction (include/gsr_densify.h).
//
//   plan:   (1) a workgroup of 256 threads counts (K, C, S, bad) over GSR_DENSIFY_PLAN_ROWS rows, a thread four consecutive rows;
//           (2) one workgroup scans the workgroup totals in index order, GSR_DENSIFY_SCAN_THREADS at a time with a running carry, and
//           leaves the exclusive bases where the totals were.  Integer sums: nothing depends on an order, and the order is fixed anyway.
//   apply:  (1) the map: the grid of the count kernel again; every workgroup scans its own threads' counts from its base and each source
//           row writes its one or two entries of src_of -- a survivor at Kbase + k, a clone copy at K + Cbase + c, the two children of a
//           split row at K + C + Sbase + s and S further on.  Threads and their rows are in index order, so every class comes out in
//           source order, and no two rows write one entry.  (2) one launch per group over the group's output words, a workgroup 1 024
//           consecutive words, lanes on consecutive words: out[d row + c] = in[src_of[d] row + c].  The kind of row d follows from its
//           position: a survivor below K (moments copied), new from K on (moments +0.0, the parameter +0.0 under zero_new), a child
//           from K + C on, whose noise row is d - (K + C).  The children's arithmetic runs in the xyz and the scale group's launch.
// No atomics, no LDS beyond the scans' wave totals, and order comes from launch boundaries only.  Indices are 32-bit: api.hip refuses
// sizes beyond that.  Counts that are not the plan's cannot make an access leave a tensor: the map writes a class's entry only below
// that class's count, and the copy skips an output row whose entry is not a row of the input.
#include "gsr_internal.h"
#include "../../include/gsr_densify.h"

#define GSR_DENSIFY_THREADS 256
#define GSR_DENSIFY_ROWS_PER_THREAD (GSR_DENSIFY_PLAN_ROWS / GSR_DENSIFY_THREADS)
#define GSR_DENSIFY_WORDS_PER_THREAD 4
#define GSR_DENSIFY_WG_WORDS (GSR_DENSIFY_THREADS * GSR_DENSIFY_WORDS_PER_THREAD)
static_assert(GSR_DENSIFY_THREADS == 256 && GSR_DENSIFY_SCAN_THREADS == 256, "the scans below fold four waves");
static_assert(GSR_DENSIFY_SPLIT_N == 2, "the map writes two children");

// (a, b, c): the thread's counts in, their exclusive prefix over the workgroup's threads out; tot: the workgroup's totals.
// wsum is free again on return.
__device__ __forceinline__ void gsr_densify_block_scan(int& a, int& b, int& c, int (*wsum)[3], int tot[3])
{
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	int ia = a, ib = b, ic = c;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) {
		const int ta = __shfl_up(ia, off, 64), tb = __shfl_up(ib, off, 64), tc = __shfl_up(ic, off, 64);
		if (lane >= off) { ia += ta; ib += tb; ic += tc; }
	}
	if (lane == 63) { wsum[w][0] = ia; wsum[w][1] = ib; wsum[w][2] = ic; }
	__syncthreads();
	int ba = 0, bb = 0, bc = 0;
	tot[0] = tot[1] = tot[2] = 0;
#pragma unroll
	for (int k = 0; k < GSR_DENSIFY_THREADS / 64; k++) {
		const int xa = wsum[k][0], xb = wsum[k][1], xc = wsum[k][2];
		if (k < w) { ba += xa; bb += xb; bc += xc; }
		tot[0] += xa; tot[1] += xb; tot[2] += xc;
	}
	a = ba + ia - a; b = bb + ib - b; c = bc + ic - c;
	__syncthreads();
}

// the codes of the thread's rows; PRUNE (counted nowhere, written nowhere) past the end
__device__ __forceinline__ void gsr_densify_codes(unsigned P, const uint8_t* __restrict__ action, unsigned first, unsigned code[GSR_DENSIFY_ROWS_PER_THREAD])
{
#pragma unroll
	for (int r = 0; r < GSR_DENSIFY_ROWS_PER_THREAD; r++) code[r] = first + r < P ? (unsigned)action[first + r] : GSR_DENSIFY_PRUNE;
}

__global__ void __launch_bounds__(GSR_DENSIFY_THREADS) gsr_densify_count_kernel(unsigned P, const uint8_t* __restrict__ action, int4* __restrict__ wg_totals)
{
	__shared__ int wsum[GSR_DENSIFY_THREADS / 64][4];
	unsigned code[GSR_DENSIFY_ROWS_PER_THREAD];
	gsr_densify_codes(P, action, blockIdx.x * GSR_DENSIFY_PLAN_ROWS + threadIdx.x * GSR_DENSIFY_ROWS_PER_THREAD, code);
	int k = 0, c = 0, s = 0, bad = 0;
#pragma unroll
	for (int r = 0; r < GSR_DENSIFY_ROWS_PER_THREAD; r++) {
		k += code[r] == GSR_DENSIFY_KEEP || code[r] == GSR_DENSIFY_CLONE;
		c += code[r] == GSR_DENSIFY_CLONE;
		s += code[r] == GSR_DENSIFY_SPLIT;
		bad += code[r] > GSR_DENSIFY_SPLIT;
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		k += __shfl_down(k, off, 64); c += __shfl_down(c, off, 64); s += __shfl_down(s, off, 64); bad += __shfl_down(bad, off, 64);
	}
	if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6][0] = k; wsum[threadIdx.x >> 6][1] = c; wsum[threadIdx.x >> 6][2] = s; wsum[threadIdx.x >> 6][3] = bad; }
	__syncthreads();
	if (threadIdx.x == 0)
		wg_totals[blockIdx.x] = make_int4(wsum[0][0] + wsum[1][0] + wsum[2][0] + wsum[3][0], wsum[0][1] + wsum[1][1] + wsum[2][1] + wsum[3][1],
		                                  wsum[0][2] + wsum[1][2] + wsum[2][2] + wsum[3][2], wsum[0][3] + wsum[1][3] + wsum[2][3] + wsum[3][3]);
}

// one workgroup: wg[i] = the exclusive sums of (K, C, S) over the workgroups before i, totals = {K, C, S, bad}
__global__ void __launch_bounds__(GSR_DENSIFY_SCAN_THREADS) gsr_densify_scan_kernel(unsigned n, int4* __restrict__ wg, int* __restrict__ totals)
{
	__shared__ int wsum[GSR_DENSIFY_SCAN_THREADS / 64][3];
	__shared__ int wbad[GSR_DENSIFY_SCAN_THREADS / 64];
	int carry[3] = {0, 0, 0}, bad = 0;
	for (unsigned first = 0; first < n; first += GSR_DENSIFY_SCAN_THREADS) {
		const unsigned i = first + threadIdx.x;
		const int4 t = i < n ? wg[i] : make_int4(0, 0, 0, 0);
		int a = t.x, b = t.y, c = t.z, tot[3];
		gsr_densify_block_scan(a, b, c, wsum, tot);
		if (i < n) wg[i] = make_int4(carry[0] + a, carry[1] + b, carry[2] + c, 0);
		carry[0] += tot[0]; carry[1] += tot[1]; carry[2] += tot[2];
		bad += t.w;
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
	if ((threadIdx.x & 63) == 0) wbad[threadIdx.x >> 6] = bad;
	__syncthreads();
	if (threadIdx.x == 0) {
		totals[0] = carry[0]; totals[1] = carry[1]; totals[2] = carry[2];
		totals[3] = wbad[0] + wbad[1] + wbad[2] + wbad[3];
	}
}

__global__ void __launch_bounds__(GSR_DENSIFY_THREADS) gsr_densify_map_kernel(unsigned P, unsigned K, unsigned C, unsigned S, const uint8_t* __restrict__ action,
                                                                              const int4* __restrict__ wg_base, int* __restrict__ src_of)
{
	__shared__ int wsum[GSR_DENSIFY_THREADS / 64][3];
	const unsigned first = blockIdx.x * GSR_DENSIFY_PLAN_ROWS + threadIdx.x * GSR_DENSIFY_ROWS_PER_THREAD;
	unsigned code[GSR_DENSIFY_ROWS_PER_THREAD];
	gsr_densify_codes(P, action, first, code);
	int k = 0, c = 0, s = 0, tot[3];
#pragma unroll
	for (int r = 0; r < GSR_DENSIFY_ROWS_PER_THREAD; r++) {
		k += code[r] == GSR_DENSIFY_KEEP || code[r] == GSR_DENSIFY_CLONE;
		c += code[r] == GSR_DENSIFY_CLONE;
		s += code[r] == GSR_DENSIFY_SPLIT;
	}
	gsr_densify_block_scan(k, c, s, wsum, tot);
	const int4 base = wg_base[blockIdx.x];
	unsigned ik = (unsigned)base.x + (unsigned)k, ic = (unsigned)base.y + (unsigned)c, is = (unsigned)base.z + (unsigned)s;
#pragma unroll
	for (int r = 0; r < GSR_DENSIFY_ROWS_PER_THREAD; r++) {
		const int i = (int)(first + r);
		if (code[r] == GSR_DENSIFY_KEEP || code[r] == GSR_DENSIFY_CLONE) {
			if (ik < K) src_of[ik] = i;
			ik++;
		}
		if (code[r] == GSR_DENSIFY_CLONE) {
			if (ic < C) src_of[K + ic] = i;
			ic++;
		}
		if (code[r] == GSR_DENSIFY_SPLIT) {
			if (is < S) { src_of[K + C + is] = i; src_of[K + C + S + is] = i; }
			is++;
		}
	}
}

enum { GSR_DENSIFY_PLAIN = 0, GSR_DENSIFY_XYZ = 1, GSR_DENSIFY_SCALE = 2 };

struct GsrDensifyCopy {
	const uint32_t *in, *in_m, *in_v;     // [P][row]; the moments both NULL or both given
	uint32_t *out, *out_m, *out_v;        // [Pout][row]
	const float *scaling, *rotation;      // the inputs of the xyz group's children: [P][3], [P][4]
	const float* noise;                   // [2 S][3]
	const int* src_of;                    // [Pout]
	unsigned P, K, KC, row, words;        // KC = K + C: the first child; words = Pout * row
	unsigned magic, shift;                // gsr_densify_div by row
	int zero_new;
};

// component c of R(q / |q|) (exp(ls) * n) for source row i and noise row e, complete in fp32
__device__ __forceinline__ float gsr_densify_displacement(const GsrDensifyCopy& a, unsigned i, unsigned e, unsigned c)
{
	const float qin[4] = {a.rotation[4 * i], a.rotation[4 * i + 1], a.rotation[4 * i + 2], a.rotation[4 * i + 3]};
	float q[4];
	gsr_act_normalize4(qin, q);
	const GsrMat3 R = gsr_build_R(q[0], q[1], q[2], q[3]);
	const float t0 = gsr_act_exp(a.scaling[3 * i]) * a.noise[3 * e], t1 = gsr_act_exp(a.scaling[3 * i + 1]) * a.noise[3 * e + 1],
	            t2 = gsr_act_exp(a.scaling[3 * i + 2]) * a.noise[3 * e + 2];
	const float d0 = R.m[0][0] * t0 + R.m[0][1] * t1 + R.m[0][2] * t2;
	const float d1 = R.m[1][0] * t0 + R.m[1][1] * t1 + R.m[1][2] * t2;
	const float d2 = R.m[2][0] * t0 + R.m[2][1] * t1 + R.m[2][2] * t2;
	return c == 0 ? d0 : c == 1 ? d1 : d2;
}

// w / row for every 32-bit w by one multiplication (Granlund and Montgomery): with shift = ceil(log2 row) and 2^32 + magic =
// ceil(2^(32 + shift) / row), which lies in [2^32, 2^33), floor(w / row) = (w + floor(w magic / 2^32)) >> shift.
__device__ __forceinline__ unsigned gsr_densify_div(unsigned w, unsigned magic, unsigned shift)
{
	return (unsigned)(((unsigned long long)__umulhi(w, magic) + w) >> shift);
}

// A thread takes GSR_DENSIFY_WORDS_PER_THREAD words a workgroup's width apart: first every map entry is requested, then every word,
// then the stores follow, so that a wave has up to sixteen loads in flight.
template <int KIND>
__global__ void __launch_bounds__(GSR_DENSIFY_THREADS) gsr_densify_copy_kernel(GsrDensifyCopy a)
{
	const unsigned row = a.row;
	unsigned d[GSR_DENSIFY_WORDS_PER_THREAD], src[GSR_DENSIFY_WORDS_PER_THREAD], from[GSR_DENSIFY_WORDS_PER_THREAD];
	uint32_t v[GSR_DENSIFY_WORDS_PER_THREAD], m1[GSR_DENSIFY_WORDS_PER_THREAD], m2[GSR_DENSIFY_WORDS_PER_THREAD];
	const unsigned w0 = blockIdx.x * GSR_DENSIFY_WG_WORDS + threadIdx.x;
#pragma unroll
	for (int u = 0; u < GSR_DENSIFY_WORDS_PER_THREAD; u++) {
		const unsigned w = w0 + u * GSR_DENSIFY_THREADS;
		d[u] = gsr_densify_div(w, a.magic, a.shift);
		src[u] = w < a.words ? (unsigned)a.src_of[d[u]] : 0xffffffffu;   // counts that were not the plan's: an entry that is no input row is skipped
	}
#pragma unroll
	for (int u = 0; u < GSR_DENSIFY_WORDS_PER_THREAD; u++) {
		const unsigned w = w0 + u * GSR_DENSIFY_THREADS;
		const bool live = src[u] < a.P, survivor = d[u] < a.K;
		from[u] = live ? src[u] * row + (w - d[u] * row) : 0u;
		v[u] = live && (survivor || !a.zero_new) ? a.in[from[u]] : 0u;
		m1[u] = a.in_m && live && survivor ? a.in_m[from[u]] : 0u;
		m2[u] = a.in_m && live && survivor ? a.in_v[from[u]] : 0u;
	}
#pragma unroll
	for (int u = 0; u < GSR_DENSIFY_WORDS_PER_THREAD; u++) {
		const unsigned w = w0 + u * GSR_DENSIFY_THREADS;
		if (src[u] >= a.P) continue;
		if (KIND != GSR_DENSIFY_PLAIN && d[u] >= a.KC && !a.zero_new) {
			if (KIND == GSR_DENSIFY_XYZ)   // the displacement is complete before it meets the position
				v[u] = __float_as_uint(__uint_as_float(v[u]) + gsr_densify_displacement(a, src[u], d[u] - a.KC, w - d[u] * row));
			else
				v[u] = __float_as_uint((float)((double)__uint_as_float(v[u]) - GSR_DENSIFY_LOG_SHRINK));
		}
		a.out[w] = v[u];
		if (a.in_m) { a.out_m[w] = m1[u]; a.out_v[w] = m2[u]; }
	}
}

// ---- host side ----
long long gsr_densify_plan_blocks(int P) { return ((long long)P + GSR_DENSIFY_PLAN_ROWS - 1) / GSR_DENSIFY_PLAN_ROWS; }
long long gsr_densify_copy_blocks(long long words) { return (words + GSR_DENSIFY_WG_WORDS - 1) / GSR_DENSIFY_WG_WORDS; }
size_t gsr_densify_scratch_size(int P) { return gsr_align_up((size_t)gsr_densify_plan_blocks(P) * sizeof(int4)); }

void gsr_launch_densify_plan(int P, const uint8_t* action, void* scratch, int32_t* totals, hipStream_t s)
{
	GsrProfScope p(s, "densify_plan");
	const unsigned blocks = (unsigned)gsr_densify_plan_blocks(P);
	hipLaunchKernelGGL(gsr_densify_count_kernel, dim3(blocks), dim3(GSR_DENSIFY_THREADS), 0, s, (unsigned)P, action, (int4*)scratch);
	hipLaunchKernelGGL(gsr_densify_scan_kernel, dim3(1), dim3(GSR_DENSIFY_SCAN_THREADS), 0, s, blocks, (int4*)scratch, (int*)totals);
}

void gsr_launch_densify_apply(const gsr_densify_args& a, hipStream_t s)
{
	GsrProfScope p(s, "densify_apply");
	const unsigned P = (unsigned)a.P, K = (unsigned)a.K, C = (unsigned)a.C, S = (unsigned)a.S, Pout = K + C + GSR_DENSIFY_SPLIT_N * S;
	hipLaunchKernelGGL(gsr_densify_map_kernel, dim3((unsigned)gsr_densify_plan_blocks(a.P)), dim3(GSR_DENSIFY_THREADS), 0, s, P, K, C, S, a.action,
	                   (const int4*)a.scratch, (int*)a.src_of);
	for (int g = 0; g < a.ngroups; g++) {
		const gsr_densify_group& grp = a.groups[g];
		if (grp.row == 0) continue;
		GsrDensifyCopy t = {};
		t.in = (const uint32_t*)grp.param; t.in_m = (const uint32_t*)grp.exp_avg; t.in_v = (const uint32_t*)grp.exp_avg_sq;
		t.out = (uint32_t*)grp.out_param; t.out_m = (uint32_t*)grp.out_exp_avg; t.out_v = (uint32_t*)grp.out_exp_avg_sq;
		t.src_of = (const int*)a.src_of;
		t.P = P; t.K = K; t.KC = K + C; t.row = (unsigned)grp.row; t.words = Pout * (unsigned)grp.row; t.zero_new = grp.zero_new;
		while ((1ull << t.shift) < (unsigned long long)t.row) t.shift++;
		t.magic = (unsigned)((((1ull << (32 + t.shift)) + t.row - 1) / t.row) - (1ull << 32));
		const dim3 grid((unsigned)gsr_densify_copy_blocks((long long)t.words)), block(GSR_DENSIFY_THREADS);
		if (S > 0 && g == a.xyz_group) {
			t.scaling = (const float*)a.groups[a.scale_group].param; t.rotation = (const float*)a.groups[a.rotation_group].param; t.noise = a.noise;
			hipLaunchKernelGGL(gsr_densify_copy_kernel<GSR_DENSIFY_XYZ>, grid, block, 0, s, t);
		} else if (S > 0 && g == a.scale_group) {
			hipLaunchKernelGGL(gsr_densify_copy_kernel<GSR_DENSIFY_SCALE>, grid, block, 0, s, t);
		} else {
			hipLaunchKernelGGL(gsr_densify_copy_kernel<GSR_DENSIFY_PLAIN>, grid, block, 0, s, t);
		}
	}
}
