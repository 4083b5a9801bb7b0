// knn_graph.hip -- exact K-nearest-neighbour search (1 <= K <= 32, self-set and two-set), the reverse adjacency of its index table
// and a neighbour gather whose backward is a fixed-order sum (include/gsr_knn.h; compiled with -ffp-contract=off as knn.hip).
//
// The search is knn.hip's: the reference points once in Morton order as float4 {x, y, z, original index}, 256-point boxes and
// 4096-point super boxes, one wave per 64 spatially coherent queries, candidates through scalar loads at a wave-uniform address.
// What differs is the lane's state.  A lane keeps its K best as 64-bit keys {distance bits : index}: squared distances are never
// negative, so their bit patterns order as unsigned integers, and one unsigned 64-bit comparison IS the lexicographic
// (distance, index) rule -- candidates arrive in Morton order, so the index has to take part.  The keys are ascending in registers
// that only compile-time constants index.  A candidate costs the distance and one comparison with the K-th key; the insertion chain
// (one compare and four selects per place) runs only when some lane of the wave accepts the candidate.
//   * an empty place holds {+inf : 0x7fffffff}, above every real pair, and leaves as (+inf, -1);
//   * a NaN distance has a bit pattern above +inf and is never accepted; every loop has fixed bounds, so the search ends whatever the
//     coordinates hold;
//   * a box is skipped only when its lower bound is strictly greater than the K-th distance (equal distances may still win on the
//     index); while a lane has fewer than K neighbours that distance is +inf and nothing is skipped.
// The radius starts from the wave's own box: in the self-set form the box its queries lie in, in the two-set form the box that holds
// the place of the wave's first query in the sorted codes (a binary search, wave-uniform).
#include "gsr_knn_common.h"

#define GSR_KNN_EMPTY 0x7f8000007fffffffull   // {+inf : INT_MAX}

template <int KI>
__device__ __forceinline__ void gsr_knng_scan_box(int P, int b, int self, float4 me, const float4* __restrict__ sorted, uint64_t (&best)[KI])
{
	const int lo = b * GSR_KNN_BOX, hi = min(P, lo + GSR_KNN_BOX);
	for (int j = lo; j < hi; j++) {   // uniform index: candidates arrive through scalar loads
		const float4 c = sorted[j];
		const float dx = c.x - me.x, dy = c.y - me.y, dz = c.z - me.z;
		const float d = dx * dx + dy * dy + dz * dz;
		uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (uint64_t)__float_as_uint(c.w);
		const bool take = j != self && key < best[KI - 1];
		if (__any(take)) {
			if (!take) key = ~0ull;   // falls through the chain without a change
#pragma unroll
			for (int k = 0; k < KI; k++) {
				const bool less = key < best[k];
				const uint64_t lo64 = less ? key : best[k];
				key = less ? best[k] : key;
				best[k] = lo64;
			}
		}
	}
}

// radius a lane still accepts: the K-th distance (+inf while places are empty)
template <int KI>
__device__ __forceinline__ float gsr_knng_radius(const uint64_t (&best)[KI]) { return __uint_as_float((uint32_t)(best[KI - 1] >> 32)); }

// TWO = false: the queries are the sorted reference points themselves (qsorted == sorted, Q == P, workgroup b = box b).
// TWO = true: qsorted holds the queries in the Morton order of their cells inside the reference bounds, qcodes their sorted codes.
template <int KI, bool TWO>
__global__ void __launch_bounds__(256) gsr_knng_search_kernel(int P, int Q, int K, const float4* __restrict__ sorted, const float4* __restrict__ qsorted,
                                                              const uint32_t* __restrict__ codes, const uint32_t* __restrict__ qcodes,
                                                              const GsrKnnBox* __restrict__ boxes, const GsrKnnBox* __restrict__ supers, int nb, int ns,
                                                              float* __restrict__ dist2, int* __restrict__ idx)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	const bool active = i < Q;
	const float4 me = active ? qsorted[i] : make_float4(0.f, 0.f, 0.f, 0.f);
	uint64_t best[KI];
#pragma unroll
	for (int k = 0; k < KI; k++) best[k] = GSR_KNN_EMPTY;

	// the wave's query bounds
	GsrKnnBox q;
	q.mnx = gsr_wave_min(active ? me.x : FLT_MAX); q.mny = gsr_wave_min(active ? me.y : FLT_MAX); q.mnz = gsr_wave_min(active ? me.z : FLT_MAX);
	q.mxx = gsr_wave_max(active ? me.x : -FLT_MAX); q.mxy = gsr_wave_max(active ? me.y : -FLT_MAX); q.mxz = gsr_wave_max(active ? me.z : -FLT_MAX);

	int own = blockIdx.x;  // GSR_KNN_BOX == workgroup size: the wave's own box
	if (TWO) {
		// the code of the wave's first query (clamped for a wave past the end, whose lanes are all idle) -> its place in the
		// sorted reference codes
		const uint32_t code = qcodes[min((int)(blockIdx.x * 256 + (threadIdx.x & ~63u)), Q - 1)];
		int lo = 0, hi = P;   // first place whose code is not below `code`
		while (lo < hi) {
			const int mid = lo + (hi - lo) / 2;
			if (codes[mid] < code) lo = mid + 1; else hi = mid;
		}
		own = __builtin_amdgcn_readfirstlane(min(lo, P - 1) / GSR_KNN_BOX);
	}
	const int self = TWO ? -1 : i;
	if (active) gsr_knng_scan_box<KI>(P, own, self, me, sorted, best);
	float wave_r = gsr_wave_max(active ? gsr_knng_radius<KI>(best) : -1.f);  // largest radius any lane still accepts

	for (int s = 0; s < ns; s++) {
		const GsrKnnBox S = supers[s];
		if (gsr_box_box_dist2(S, q) > wave_r) continue;                        // wave-uniform
		for (int b = s * GSR_KNN_SUPER; b < min(nb, (s + 1) * GSR_KNN_SUPER); b++) {
			if (b == own) continue;
			const GsrKnnBox B = boxes[b];
			if (gsr_box_box_dist2(B, q) > wave_r) continue;                    // wave-uniform
			const float d = gsr_point_box_dist2(B, me.x, me.y, me.z);
			const bool need = active && !(d > gsr_knng_radius<KI>(best));
			if (need) gsr_knng_scan_box<KI>(P, b, self, me, sorted, best);
			wave_r = gsr_wave_max(active ? gsr_knng_radius<KI>(best) : -1.f);
		}
	}
	if (active) {
		const size_t row = (size_t)__float_as_uint(me.w) * (size_t)K;
#pragma unroll
		for (int k = 0; k < KI; k++)
			if (k < K) {
				const uint32_t j = (uint32_t)best[k];
				dist2[row + k] = __uint_as_float((uint32_t)(best[k] >> 32));
				idx[row + k] = j == 0x7fffffffu ? -1 : (int)j;
			}
	}
}

template <int KI>
static void gsr_knng_launch(bool two, int nq_blocks, hipStream_t s, int P, int Q, int K, const float4* sorted, const float4* qsorted, const uint32_t* codes,
                            const uint32_t* qcodes, const GsrKnnBox* boxes, const GsrKnnBox* supers, int nb, int ns, float* dist2, int* idx)
{
	if (two)
		hipLaunchKernelGGL((gsr_knng_search_kernel<KI, true>), dim3(nq_blocks), dim3(256), 0, s, P, Q, K, sorted, qsorted, codes, qcodes, boxes, supers, nb, ns, dist2, idx);
	else
		hipLaunchKernelGGL((gsr_knng_search_kernel<KI, false>), dim3(nq_blocks), dim3(256), 0, s, P, Q, K, sorted, qsorted, codes, qcodes, boxes, supers, nb, ns, dist2, idx);
}

// scratch: the reference set's areas, then the query set's (two-set form)
size_t gsr_knn_search_scratch_size(int P, int Q)
{
	if (P <= 0) return 0;
	return gsr_knn_carve(nullptr, P).total + (Q > 0 ? gsr_knn_carve(nullptr, Q).total : 0);
}

void gsr_launch_knn_search(int P, const float* points, int Q, const float* queries, int K, float* dist2, int* idx, void* scratch, hipStream_t s)
{
	GsrKnnScratch k = gsr_knn_carve(scratch, P);
	const int nb = (P + GSR_KNN_BOX - 1) / GSR_KNN_BOX, ns = (nb + GSR_KNN_SUPER - 1) / GSR_KNN_SUPER;
	GsrProfScope p(s, "knn_search");
	gsr_knn_cloud_bounds(P, points, k, s);
	const uint32_t* codes = gsr_knn_morton_order(P, points, k.bounds, k, s);
	const float4* qsorted = k.sorted;
	const uint32_t* qcodes = codes;
	if (queries) {
		GsrKnnScratch kq = gsr_knn_carve((char*)scratch + k.total, Q);
		qcodes = gsr_knn_morton_order(Q, queries, k.bounds, kq, s);
		qsorted = kq.sorted;
	}
	const int nqb = (Q + 255) / 256;
	const bool two = queries != nullptr;
	if (K <= 4) gsr_knng_launch<4>(two, nqb, s, P, Q, K, k.sorted, qsorted, codes, qcodes, k.boxes, k.supers, nb, ns, dist2, idx);
	else if (K <= 8) gsr_knng_launch<8>(two, nqb, s, P, Q, K, k.sorted, qsorted, codes, qcodes, k.boxes, k.supers, nb, ns, dist2, idx);
	else if (K <= 16) gsr_knng_launch<16>(two, nqb, s, P, Q, K, k.sorted, qsorted, codes, qcodes, k.boxes, k.supers, nb, ns, dist2, idx);
	else gsr_knng_launch<32>(two, nqb, s, P, Q, K, k.sorted, qsorted, codes, qcodes, k.boxes, k.supers, nb, ns, dist2, idx);
}

// ---- reverse adjacency: a stable sort of the edge ids by target ---------------------------------------------
// key = the target, P for an entry that names none (-1; a value outside [-1, P) counts as none too, so nothing reads out of bounds)
__global__ void __launch_bounds__(256) gsr_knng_edge_keys_kernel(int E, int P, const int* __restrict__ idx, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
	const int e = blockIdx.x * 256 + threadIdx.x;
	if (e >= E) return;
	const int j = idx[e];
	keys[e] = (j >= 0 && j < P) ? (uint32_t)j : (uint32_t)P;
	vals[e] = (uint32_t)e;
}

// offsets[j] = the first sorted place whose key is not below j, j = 0 .. P; offsets[P] = the number of valid edges
__global__ void __launch_bounds__(256) gsr_knng_offsets_kernel(int E, int P, const uint32_t* __restrict__ keys, int* __restrict__ offsets, int* __restrict__ num_valid)
{
	const int j = blockIdx.x * 256 + threadIdx.x;
	if (j > P) return;
	int lo = 0, hi = E;
	while (lo < hi) {
		const int mid = lo + (hi - lo) / 2;
		if (keys[mid] < (uint32_t)j) lo = mid + 1; else hi = mid;
	}
	offsets[j] = lo;
	if (j == P && num_valid) *num_valid = lo;
}

__global__ void __launch_bounds__(256) gsr_knng_zero_offsets_kernel(int P, int* __restrict__ offsets, int* __restrict__ num_valid)
{
	const int j = blockIdx.x * 256 + threadIdx.x;
	if (j <= P) offsets[j] = 0;
	if (j == 0 && num_valid) *num_valid = 0;
}

static int gsr_knng_key_bits(int P)   // bits of the largest key, P
{
	int bits = 1;
	while (bits < 31 && ((unsigned)P >> bits) != 0u) bits++;
	return bits;
}

struct GsrKnnGraphScratch { uint32_t *keys, *keys_alt, *vals_alt; void* table; size_t total; };

static GsrKnnGraphScratch gsr_knng_carve(void* base, int E)
{
	size_t off = 0;
	auto take = [&](size_t bytes) { void* p = (char*)base + off; off += gsr_align_up(bytes); return p; };
	GsrKnnGraphScratch g;
	g.keys = (uint32_t*)take(4 * (size_t)E); g.keys_alt = (uint32_t*)take(4 * (size_t)E);
	g.vals_alt = (uint32_t*)take(4 * (size_t)E);
	g.table = take(gsr_radix_table_bytes((size_t)E));
	g.total = off;
	return g;
}

size_t gsr_knn_graph_scratch_size(int E, int P) { return (E > 0 && P > 0) ? gsr_knng_carve(nullptr, E).total : 0; }

// edges has room for E ids; the first offsets[P] are written
void gsr_launch_knn_graph_build(int E, const int* idx, int P, int* offsets, int* edges, int* num_valid, void* scratch, hipStream_t s)
{
	GsrProfScope p(s, "knn_graph_build");
	if (E == 0 || P == 0) {
		hipLaunchKernelGGL(gsr_knng_zero_offsets_kernel, dim3(P / 256 + 1), dim3(256), 0, s, P, offsets, num_valid);
		return;
	}
	GsrKnnGraphScratch g = gsr_knng_carve(scratch, E);
	const int bits = gsr_knng_key_bits(P);
	// the sort ends in its first pair of buffers after an even number of passes, in its second after an odd one: `edges` is that one
	const bool even = gsr_radix_num_passes(bits) % 2 == 0;
	uint32_t* v0 = even ? (uint32_t*)edges : g.vals_alt;
	uint32_t* v1 = even ? g.vals_alt : (uint32_t*)edges;
	hipLaunchKernelGGL(gsr_knng_edge_keys_kernel, dim3((E + 255) / 256), dim3(256), 0, s, E, P, idx, g.keys, v0);
	int in_first = 1;
	gsr_radix_sort_u32(g.keys, v0, g.keys_alt, v1, (size_t)E, bits, g.table, &in_first, 1, 4, s);
	hipLaunchKernelGGL(gsr_knng_offsets_kernel, dim3(P / 256 + 1), dim3(256), 0, s, E, P, in_first ? g.keys : g.keys_alt, offsets, num_valid);
}

// ---- gather and its backward --------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gsr_knng_gather_kernel(size_t total, int C, const float* __restrict__ x, const int* __restrict__ idx, float* __restrict__ out)
{
	const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= total) return;
	const size_t e = t / (size_t)C;
	const int c = (int)(t - e * (size_t)C);
	const int j = idx[e];
	out[t] = j >= 0 ? x[(size_t)j * (size_t)C + c] : 0.f;
}

// One thread owns grad_x[j][c] and adds its row's edges in ascending edge order: the sequential fp32 sum, no atomics.  The loads of
// four edges are issued together; the additions keep their order.  A long row (every query pointing at one target) would otherwise pay
// two dependent memory round trips per four edges: from GSR_KNNG_LONG edges on, the values of sixteen edges and the ids of the next
// sixteen are in flight while the sixteen before them are added, still one by one in edge order.
#define GSR_KNNG_BATCH 16
#define GSR_KNNG_LONG (4 * GSR_KNNG_BATCH)
__global__ void __launch_bounds__(256) gsr_knng_gather_backward_kernel(size_t total, int C, const int* __restrict__ offsets, const int* __restrict__ edges,
                                                                        const float* __restrict__ grad_out, float* __restrict__ grad_x)
{
	const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= total) return;
	const size_t j = t / (size_t)C;
	const int c = (int)(t - j * (size_t)C);
	const int lo = offsets[j], hi = offsets[j + 1];
	float acc = 0.f;
	int i = lo;
	if (hi - lo >= GSR_KNNG_LONG) {
		int e[GSR_KNNG_BATCH];
#pragma unroll
		for (int k = 0; k < GSR_KNNG_BATCH; k++) e[k] = edges[i + k];
		for (; i + 2 * GSR_KNNG_BATCH <= hi; i += GSR_KNNG_BATCH) {   // e = the ids of [i, i + BATCH); the next batch lies inside the row
			float v[GSR_KNNG_BATCH];
#pragma unroll
			for (int k = 0; k < GSR_KNNG_BATCH; k++) v[k] = grad_out[(size_t)e[k] * (size_t)C + c];
#pragma unroll
			for (int k = 0; k < GSR_KNNG_BATCH; k++) e[k] = edges[i + GSR_KNNG_BATCH + k];
#pragma unroll
			for (int k = 0; k < GSR_KNNG_BATCH; k++) acc += v[k];
		}
#pragma unroll
		for (int k = 0; k < GSR_KNNG_BATCH; k++) acc += grad_out[(size_t)e[k] * (size_t)C + c];   // the batch whose ids are loaded
		i += GSR_KNNG_BATCH;
	}
	for (; i + 4 <= hi; i += 4) {
		const float a0 = grad_out[(size_t)edges[i] * (size_t)C + c], a1 = grad_out[(size_t)edges[i + 1] * (size_t)C + c];
		const float a2 = grad_out[(size_t)edges[i + 2] * (size_t)C + c], a3 = grad_out[(size_t)edges[i + 3] * (size_t)C + c];
		acc += a0; acc += a1; acc += a2; acc += a3;
	}
	for (; i < hi; i++) acc += grad_out[(size_t)edges[i] * (size_t)C + c];
	grad_x[t] = acc;
}

void gsr_launch_knn_gather(int64_t E, int C, const float* x, const int* idx, float* out, hipStream_t s)
{
	const size_t total = (size_t)E * (size_t)C;
	GsrProfScope p(s, "knn_gather");
	hipLaunchKernelGGL(gsr_knng_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, total, C, x, idx, out);
}

void gsr_launch_knn_gather_backward(int P, int C, const int* offsets, const int* edges, const float* grad_out, float* grad_x, hipStream_t s)
{
	const size_t total = (size_t)P * (size_t)C;
	GsrProfScope p(s, "knn_gather_bwd");
	hipLaunchKernelGGL(gsr_knng_gather_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, total, C, offsets, edges, grad_out, grad_x);
}
