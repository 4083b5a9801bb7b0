// tsdf.hip -- TSDF fusion of depth maps and marching tetrahedra over the fused field (include/gsr_tsdf.h).
//
//   integrate: a workgroup takes a brick of 8 x 8 x 4 nodes, a wave 8 x 8 x 1 of them, a thread one node, whose position and sums stay in
//              registers while it walks the cameras.  The record's address depends on the loop counter alone: wave-uniform, fetched with
//              scalar loads, as in the sweep of filter3d.hip.  Per node and camera: three fma chains, one reciprocal, two fmas and four
//              comparisons up to the pixel; one gathered load of the depth (the wave's 64 nodes project to neighbouring pixels); the
//              cuts; one to four gathered loads and as many fmas where the node is touched.  The planes are read once and written once
//              where touched.  A per-wave test of the cameras against the wave's bounding sphere (a ballot of 64
//              tests, the walk over its set bits) was tried and measured 2 to 8 % slower with the same bits, also where each camera
//              sees a sixth of the volume: a pair behind the camera or beside the image leaves the loop after a few instructions
//              anyway.
//   mesh plan: a thread per node n reads the node and its seven upper neighbours -- the corners of cell n -- and forms the node's
//              7-bit crossing mask (stored) and the cell's triangle count; the workgroup's two totals go to scratch; one workgroup of
//              1 024 threads scans them in index order, four a thread, with a running 64-bit carry.
//   mesh emit: (1) a thread per node: the workgroup scans its masks' populations from its base, stores every node's first vertex id
//              and writes the node's vertices, evaluated in double and rounded once.  (2) a thread per cell, which reads the cell's
//              corners only where its node's mask is not 0 (no crossing at the node: no triangle in the cell): the workgroup scans
//              its triangle counts again and each cell writes its triangles; a vertex id is the owner's first id plus the rank of the
//              edge kind in the owner's mask.  Order comes from index order and launch boundaries only: no atomics.
// A write happens only below the caller's V and F and a read only inside the grid: counts that are not the plan's leave no tensor.
// Indices are 32-bit: api.hip refuses sizes beyond that.
#include "gsr_internal.h"
#include "../../include/gsr_tsdf.h"

#define GSR_TSDF_WAVES (GSR_TSDF_THREADS / 64)
#define GSR_TSDF_SCAN_THREADS 1024
#define GSR_TSDF_SCAN_PER_THREAD 4
#define GSR_TSDF_HEAD 16   // bytes in front of the workgroup totals: {V, F} as two 64-bit integers
static_assert(GSR_TSDF_BRICK_X * GSR_TSDF_BRICK_Y == 64 && GSR_TSDF_BRICK_X * GSR_TSDF_BRICK_Y * GSR_TSDF_BRICK_Z == GSR_TSDF_THREADS,
              "a wave is one z layer of the brick");

// ---- integration ----
struct GsrTsdfIntegrate {
	unsigned nx, ny, nz, bx, by;   // bx, by: bricks along x and y
	float ox, oy, oz, vs;
	float *wsum, *dsum, *csum;
	const gsr_filter3d_camera* cameras;
	int C, H, W;
	const float *depth, *color, *weight;
	float trunc, inv_trunc, depth_trunc;
};

// one camera on one node: the rule of gsr_tsdf.h, operation for operation
template <bool COLOR>
__device__ __forceinline__ void gsr_tsdf_pair(const GsrTsdfIntegrate& a, int c, float x, float y, float z, float& ws, float& ds, float (&cs)[3],
                                              bool& touched)
{
	const gsr_filter3d_camera& k = a.cameras[c];   // wave-uniform
	const float pz = fmaf(k.R[6], x, fmaf(k.R[7], y, fmaf(k.R[8], z, k.t[2])));
	if (!(pz > 0.0f)) return;
	const float px = fmaf(k.R[0], x, fmaf(k.R[1], y, fmaf(k.R[2], z, k.t[0])));
	const float py = fmaf(k.R[3], x, fmaf(k.R[4], y, fmaf(k.R[5], z, k.t[1])));
	const float r = __builtin_amdgcn_rcpf(pz);
	const float U = fmaf(px * r, k.fx, k.cx), V = fmaf(py * r, k.fy, k.cy);
	if (!((U >= 0.0f) & (U < (float)a.W) & (V >= 0.0f) & (V < (float)a.H))) return;   // a NaN is in no pixel
	const unsigned pixel = (unsigned)(int)V * (unsigned)a.W + (unsigned)(int)U;           // U, V >= 0: the conversion is the floor
	const size_t plane = (size_t)a.H * (size_t)a.W;
	const float d = a.depth[(size_t)c * plane + pixel];
	if (!((d > 0.0f) & (d <= a.depth_trunc) & (d < INFINITY))) return;
	const float sdf = d - pz;
	if (sdf < -a.trunc) return;
	const float tsdf = fminf(1.0f, sdf * a.inv_trunc);
	const float w = a.weight ? a.weight[(size_t)c * plane + pixel] : 1.0f;
	if (!((w > 0.0f) & (w < INFINITY))) return;
	ws = ws + w;
	ds = fmaf(w, tsdf, ds);
	if (COLOR) {
		const float* rgb = a.color + (size_t)c * 3 * plane + pixel;
#pragma unroll
		for (int ch = 0; ch < 3; ch++) cs[ch] = fmaf(w, rgb[(size_t)ch * plane], cs[ch]);
	}
	touched = true;
}

template <bool COLOR>
__global__ void __launch_bounds__(GSR_TSDF_THREADS) gsr_tsdf_integrate_kernel(GsrTsdfIntegrate a)
{
	const unsigned lane = threadIdx.x & 63, layer = threadIdx.x >> 6;
	const unsigned brick = blockIdx.x, bi = brick % a.bx, bj = (brick / a.bx) % a.by, bk = brick / (a.bx * a.by);
	const unsigned i = bi * GSR_TSDF_BRICK_X + (lane & 7), j = bj * GSR_TSDF_BRICK_Y + (lane >> 3), kz = bk * GSR_TSDF_BRICK_Z + layer;
	const bool live = (i < a.nx) & (j < a.ny) & (kz < a.nz);
	const unsigned node = live ? i + a.nx * (j + a.ny * kz) : 0u;
	const size_t nodes = (size_t)a.nx * a.ny * a.nz;
	const float x = fmaf((float)i, a.vs, a.ox), y = fmaf((float)j, a.vs, a.oy), z = fmaf((float)kz, a.vs, a.oz);
	float ws = 0.0f, ds = 0.0f, cs[3] = {0.0f, 0.0f, 0.0f};
	if (live) {
		ws = a.wsum[node];
		ds = a.dsum[node];
		if (COLOR) {
#pragma unroll
			for (int ch = 0; ch < 3; ch++) cs[ch] = a.csum[ch * nodes + node];
		}
	}
	bool touched = false;
	if (live) {
		for (int c = 0; c < a.C; c++) gsr_tsdf_pair<COLOR>(a, c, x, y, z, ws, ds, cs, touched);
	}
	if (touched) {
		a.wsum[node] = ws;
		a.dsum[node] = ds;
		if (COLOR) {
#pragma unroll
			for (int ch = 0; ch < 3; ch++) a.csum[ch * nodes + node] = cs[ch];
		}
	}
}

// ---- marching tetrahedra ----
// corner c of a cell: bit 0 = +x, bit 1 = +y, bit 2 = +z.  Tetrahedron T walks 0 -> A -> AB -> 7; its orientation det[e_a, e_b, e_c] is
// +1 for the even axis orders
__constant__ const unsigned char gsr_tsdf_tet_a[6] = {1, 1, 2, 2, 4, 4};
__constant__ const unsigned char gsr_tsdf_tet_ab[6] = {3, 5, 3, 6, 5, 6};
#define GSR_TSDF_ODD_TETS 0x26u   // bit T: the axis order of T is odd (xzy, yxz, zyx): second and third vertex of every triangle swap
// the rank of an edge kind by its corner difference: +x, +y, +z, +xy, +yz, +xz, +xyz
__constant__ const unsigned char gsr_tsdf_kind_rank[8] = {0, 0, 1, 3, 2, 5, 4, 6};
__constant__ const unsigned char gsr_tsdf_rank_kind[7] = {1, 2, 4, 3, 6, 5, 7};
// The sixteen cases of an even tetrahedron (bit l of the case: path corner l is inside): the edges of up to two triangles, an edge as
// lo | hi << 2 of its path corners.  One corner a apart from b < c < d: the triangle (ab, ac, ad), which looks away from a where the
// permutation (a, b, c, d) is even, reversed as needed so that it looks out of the inside.  Two inside: the sentence of gsr_tsdf.h,
// the cycle (ac, ad, bd, bc) looking outside where (a, b, c, d) is even.  (DESIGN.md 6w derives it; tests/torch_tsdf.py shares none of it.)
__constant__ const unsigned char gsr_tsdf_case[16][6] = {
	{0, 0, 0, 0, 0, 0},    {4, 8, 12, 0, 0, 0},   {4, 13, 9, 0, 0, 0},   {8, 12, 13, 8, 13, 9}, {8, 9, 14, 0, 0, 0},  {4, 14, 12, 4, 9, 14},
	{4, 13, 14, 4, 14, 8}, {12, 13, 14, 0, 0, 0}, {12, 14, 13, 0, 0, 0}, {4, 8, 14, 4, 14, 13}, {4, 14, 9, 4, 12, 14}, {8, 14, 9, 0, 0, 0},
	{8, 9, 13, 8, 13, 12}, {4, 9, 13, 0, 0, 0},   {4, 12, 8, 0, 0, 0},   {0, 0, 0, 0, 0, 0}};

struct GsrTsdfMesh {
	unsigned nx, ny, nz, nodes;
	float ox, oy, oz, vs, min_weight;
	const float *wsum, *dsum, *csum;
	int2* wg;                // [workgroups]: totals after the count, exclusive bases after the scan
	int* vbase;              // [nodes]
	unsigned char* mask;     // [nodes]
	long long* totals;       // {V, F}
	unsigned V, F;
	float *vertices, *colors;
	int* faces;
};

// what thread n knows of cell n: bit c of `valid` / `inside` for corner c (corners outside the grid are invalid)
struct GsrTsdfCell {
	unsigned i, j, k, valid, inside;
	bool whole;   // all eight corners lie in the grid
};

__device__ __forceinline__ unsigned gsr_tsdf_corner(const GsrTsdfMesh& a, unsigned n, unsigned c)
{
	return n + (c & 1u) + ((c >> 1) & 1u) * a.nx + (c >> 2) * a.nx * a.ny;
}

__device__ __forceinline__ GsrTsdfCell gsr_tsdf_cell(const GsrTsdfMesh& a, unsigned n)
{
	GsrTsdfCell q;
	q.i = n % a.nx; q.j = (n / a.nx) % a.ny; q.k = n / (a.nx * a.ny);
	const bool mx = q.i + 1 < a.nx, my = q.j + 1 < a.ny, mz = q.k + 1 < a.nz;
	q.whole = mx & my & mz;
	q.valid = q.inside = 0;
#pragma unroll
	for (unsigned c = 0; c < 8; c++) {
		const bool in_grid = ((c & 1u) == 0 || mx) && ((c & 2u) == 0 || my) && ((c & 4u) == 0 || mz);
		if (!in_grid) continue;
		const unsigned m = gsr_tsdf_corner(a, n, c);
		const float w = a.wsum[m], d = a.dsum[m];
		q.valid |= (unsigned)(w >= a.min_weight) << c;   // w > 0 there: the sign of dsum / wsum is the sign of dsum
		q.inside |= (unsigned)(d < 0.0f) << c;
	}
	return q;
}

// the node's crossing mask: bit r for the edge of kind rank r
__device__ __forceinline__ unsigned gsr_tsdf_crossings(const GsrTsdfCell& q)
{
	unsigned m = 0;
	if (!(q.valid & 1u)) return 0;
#pragma unroll
	for (unsigned r = 0; r < 7; r++) {
		const unsigned c = gsr_tsdf_rank_kind[r];
		m |= (((q.valid >> c) & 1u) & (((q.inside >> c) ^ q.inside) & 1u)) << r;
	}
	return m;
}

// the case of tetrahedron T of the cell, 0 where it emits nothing
__device__ __forceinline__ unsigned gsr_tsdf_tet_case(const GsrTsdfCell& q, unsigned T)
{
	const unsigned c1 = gsr_tsdf_tet_a[T], c2 = gsr_tsdf_tet_ab[T];
	const unsigned all = 1u | (1u << c1) | (1u << c2) | 0x80u;
	if ((q.valid & all) != all) return 0;
	const unsigned m = (q.inside & 1u) | (((q.inside >> c1) & 1u) << 1) | (((q.inside >> c2) & 1u) << 2) | (((q.inside >> 7) & 1u) << 3);
	return m == 15u ? 0u : m;
}

__device__ __forceinline__ int gsr_tsdf_case_triangles(unsigned m) { return m == 0 ? 0 : (__popc(m) == 2 ? 2 : 1); }

__device__ __forceinline__ int gsr_tsdf_cell_triangles(const GsrTsdfCell& q)
{
	int f = 0;
	if (q.whole) {
#pragma unroll
		for (unsigned T = 0; T < 6; T++) f += gsr_tsdf_case_triangles(gsr_tsdf_tet_case(q, T));
	}
	return f;
}

// (a, b): the thread's counts in, their exclusive prefix over the workgroup's threads out; tot: the workgroup's totals.  wsum is free
// again on return.
template <int WAVES>
__device__ __forceinline__ void gsr_tsdf_block_scan(int& a, int& b, int (*wsum)[2], int tot[2])
{
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	int ia = a, ib = b;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) {
		const int ta = __shfl_up(ia, off, 64), tb = __shfl_up(ib, off, 64);
		if (lane >= off) { ia += ta; ib += tb; }
	}
	if (lane == 63) { wsum[w][0] = ia; wsum[w][1] = ib; }
	__syncthreads();
	int ba = 0, bb = 0;
	tot[0] = tot[1] = 0;
#pragma unroll
	for (int k = 0; k < WAVES; k++) {
		const int xa = wsum[k][0], xb = wsum[k][1];
		if (k < w) { ba += xa; bb += xb; }
		tot[0] += xa; tot[1] += xb;
	}
	a = ba + ia - a; b = bb + ib - b;
	__syncthreads();
}

__global__ void __launch_bounds__(GSR_TSDF_THREADS) gsr_tsdf_count_kernel(GsrTsdfMesh a)
{
	__shared__ int wsum[GSR_TSDF_WAVES][2];
	const unsigned n = blockIdx.x * GSR_TSDF_THREADS + threadIdx.x;
	int v = 0, f = 0, tot[2];
	if (n < a.nodes) {
		const GsrTsdfCell q = gsr_tsdf_cell(a, n);
		const unsigned m = gsr_tsdf_crossings(q);
		a.mask[n] = (unsigned char)m;
		v = __popc(m);
		f = gsr_tsdf_cell_triangles(q);
	}
	gsr_tsdf_block_scan<GSR_TSDF_WAVES>(v, f, wsum, tot);
	if (threadIdx.x == 0) a.wg[blockIdx.x] = make_int2(tot[0], tot[1]);
}

// one workgroup: wg[i] = the exclusive sums over the workgroups before i (their low 32 bits: emit is refused where they do not fit),
// totals = {V, F}
__global__ void __launch_bounds__(GSR_TSDF_SCAN_THREADS) gsr_tsdf_scan_kernel(unsigned n, int2* __restrict__ wg, long long* __restrict__ totals)
{
	__shared__ int wsum[GSR_TSDF_SCAN_THREADS / 64][2];
	long long carry[2] = {0, 0};
	for (unsigned first = 0; first < n; first += GSR_TSDF_SCAN_THREADS * GSR_TSDF_SCAN_PER_THREAD) {
		const unsigned mine = first + threadIdx.x * GSR_TSDF_SCAN_PER_THREAD;
		int2 t[GSR_TSDF_SCAN_PER_THREAD];
		int a = 0, b = 0, tot[2];
#pragma unroll
		for (int u = 0; u < GSR_TSDF_SCAN_PER_THREAD; u++) {
			t[u] = mine + u < n ? wg[mine + u] : make_int2(0, 0);
			a += t[u].x; b += t[u].y;
		}
		gsr_tsdf_block_scan<GSR_TSDF_SCAN_THREADS / 64>(a, b, wsum, tot);
		long long ra = carry[0] + a, rb = carry[1] + b;
#pragma unroll
		for (int u = 0; u < GSR_TSDF_SCAN_PER_THREAD; u++) {
			if (mine + u < n) wg[mine + u] = make_int2((int)ra, (int)rb);
			ra += t[u].x; rb += t[u].y;
		}
		carry[0] += tot[0]; carry[1] += tot[1];
	}
	if (threadIdx.x == 0) { totals[0] = carry[0]; totals[1] = carry[1]; }
}

__global__ void __launch_bounds__(GSR_TSDF_THREADS) gsr_tsdf_vertex_kernel(GsrTsdfMesh a)
{
	__shared__ int wsum[GSR_TSDF_WAVES][2];
	const unsigned n = blockIdx.x * GSR_TSDF_THREADS + threadIdx.x;
	const bool live = n < a.nodes;
	const unsigned m = live ? a.mask[n] : 0u;
	int v = __popc(m), unused = 0, tot[2];
	gsr_tsdf_block_scan<GSR_TSDF_WAVES>(v, unused, wsum, tot);
	if (!live) return;
	unsigned id = (unsigned)a.wg[blockIdx.x].x + (unsigned)v;
	a.vbase[n] = (int)id;
	if (m == 0) return;
	const unsigned i = n % a.nx, j = (n / a.nx) % a.ny, k = n / (a.nx * a.ny);
	const double w0 = (double)a.wsum[n], v0 = (double)a.dsum[n] / w0;
	const double base[3] = {(double)i, (double)j, (double)k}, org[3] = {(double)a.ox, (double)a.oy, (double)a.oz};
	for (unsigned r = 0; r < 7; r++) {
		if (!((m >> r) & 1u)) continue;
		const unsigned c = gsr_tsdf_rank_kind[r], up = gsr_tsdf_corner(a, n, c);
		if (((c & 1u) && i + 1 >= a.nx) || ((c & 2u) && j + 1 >= a.ny) || ((c & 4u) && k + 1 >= a.nz)) continue;   // a mask that is not the plan's
		const double w1 = (double)a.wsum[up], v1 = (double)a.dsum[up] / w1;
		const double t = v0 / (v0 - v1);   // the signs differ: the denominator is not 0
		if (id < a.V) {
#pragma unroll
			for (unsigned ax = 0; ax < 3; ax++)
				a.vertices[3 * (size_t)id + ax] = (float)(org[ax] + (base[ax] + (((c >> ax) & 1u) ? t : 0.0)) * (double)a.vs);
			if (a.colors) {
#pragma unroll
				for (unsigned ch = 0; ch < 3; ch++) {
					const double c0 = (double)a.csum[(size_t)ch * a.nodes + n] / w0, c1 = (double)a.csum[(size_t)ch * a.nodes + up] / w1;
					a.colors[3 * (size_t)id + ch] = (float)(c0 + t * (c1 - c0));
				}
			}
		}
		id++;
	}
}

__global__ void __launch_bounds__(GSR_TSDF_THREADS) gsr_tsdf_face_kernel(GsrTsdfMesh a)
{
	__shared__ int wsum[GSR_TSDF_WAVES][2];
	const unsigned n = blockIdx.x * GSR_TSDF_THREADS + threadIdx.x;
	const bool live = n < a.nodes;
	// every emitting tetrahedron holds corner 0 and a valid corner on the other side of it, which is a bit of the node's own mask:
	// a node without crossings (nearly all of them) has no triangles, and its cell's corners are not read
	const bool crossed = live && a.mask[n] != 0;
	GsrTsdfCell q = {};
	if (crossed) q = gsr_tsdf_cell(a, n);
	int f = crossed ? gsr_tsdf_cell_triangles(q) : 0, unused = 0, tot[2];
	const int mine = f;
	gsr_tsdf_block_scan<GSR_TSDF_WAVES>(f, unused, wsum, tot);
	if (mine == 0) return;
	unsigned id = (unsigned)a.wg[blockIdx.x].y + (unsigned)f;
	for (unsigned T = 0; T < 6; T++) {
		const unsigned m = gsr_tsdf_tet_case(q, T);
		const int count = gsr_tsdf_case_triangles(m);
		const unsigned path[4] = {0u, gsr_tsdf_tet_a[T], gsr_tsdf_tet_ab[T], 7u};
		const bool odd = (GSR_TSDF_ODD_TETS >> T) & 1u;
		for (int tri = 0; tri < count; tri++, id++) {
			if (id >= a.F) continue;
#pragma unroll
			for (int s = 0; s < 3; s++) {
				const unsigned e = gsr_tsdf_case[m][3 * tri + (odd && s ? 3 - s : s)];
				const unsigned lo = path[e & 3u], hi = path[e >> 2];
				const unsigned owner = gsr_tsdf_corner(a, n, lo), r = gsr_tsdf_kind_rank[hi ^ lo];
				a.faces[3 * (size_t)id + s] = a.vbase[owner] + __popc((unsigned)a.mask[owner] & ((1u << r) - 1u));
			}
		}
	}
}

// ---- host side ----
static unsigned gsr_tsdf_blocks(long long nodes) { return (unsigned)((nodes + GSR_TSDF_THREADS - 1) / GSR_TSDF_THREADS); }

size_t gsr_tsdf_mesh_scratch_size(long long nodes)
{
	return (size_t)GSR_TSDF_HEAD + (size_t)gsr_tsdf_blocks(nodes) * sizeof(int2) + (size_t)nodes * 5;
}

long long gsr_tsdf_integrate_blocks(const gsr_tsdf_grid& g)
{
	const long long bx = (g.nx + GSR_TSDF_BRICK_X - 1) / GSR_TSDF_BRICK_X, by = (g.ny + GSR_TSDF_BRICK_Y - 1) / GSR_TSDF_BRICK_Y,
	                bz = (g.nz + GSR_TSDF_BRICK_Z - 1) / GSR_TSDF_BRICK_Z;
	return bx * by * bz;
}

void gsr_launch_tsdf_integrate(const gsr_tsdf_grid& g, float* wsum, float* dsum, float* csum, int C, const gsr_filter3d_camera* cameras, int H, int W,
                               const float* depth, const float* color, const float* weight, float sdf_trunc, float depth_trunc, hipStream_t s)
{
	GsrProfScope p(s, "tsdf_integrate");
	GsrTsdfIntegrate a = {};
	a.nx = (unsigned)g.nx; a.ny = (unsigned)g.ny; a.nz = (unsigned)g.nz;
	a.bx = (a.nx + GSR_TSDF_BRICK_X - 1) / GSR_TSDF_BRICK_X; a.by = (a.ny + GSR_TSDF_BRICK_Y - 1) / GSR_TSDF_BRICK_Y;
	a.ox = g.origin[0]; a.oy = g.origin[1]; a.oz = g.origin[2]; a.vs = g.voxel_size;
	a.wsum = wsum; a.dsum = dsum; a.csum = csum;
	a.cameras = cameras; a.C = C; a.H = H; a.W = W;
	a.depth = depth; a.color = csum ? color : nullptr; a.weight = weight;
	a.trunc = sdf_trunc; a.inv_trunc = (float)(1.0 / (double)sdf_trunc); a.depth_trunc = depth_trunc;
	const dim3 grid((unsigned)gsr_tsdf_integrate_blocks(g)), block(GSR_TSDF_THREADS);
	if (a.color) hipLaunchKernelGGL(gsr_tsdf_integrate_kernel<true>, grid, block, 0, s, a);
	else hipLaunchKernelGGL(gsr_tsdf_integrate_kernel<false>, grid, block, 0, s, a);
}

static GsrTsdfMesh gsr_tsdf_mesh_args(const gsr_tsdf_grid& g, const float* wsum, const float* dsum, float min_weight, void* scratch)
{
	GsrTsdfMesh a = {};
	a.nx = (unsigned)g.nx; a.ny = (unsigned)g.ny; a.nz = (unsigned)g.nz; a.nodes = a.nx * a.ny * a.nz;
	a.ox = g.origin[0]; a.oy = g.origin[1]; a.oz = g.origin[2]; a.vs = g.voxel_size; a.min_weight = min_weight;
	a.wsum = wsum; a.dsum = dsum;
	char* base = (char*)scratch;
	a.totals = (long long*)base;
	a.wg = (int2*)(base + GSR_TSDF_HEAD);
	a.vbase = (int*)(base + GSR_TSDF_HEAD + (size_t)gsr_tsdf_blocks(a.nodes) * sizeof(int2));
	a.mask = (unsigned char*)(a.vbase + a.nodes);
	return a;
}

// counts and scan, then the read-back of {V, F}: synchronises the stream
hipError_t gsr_launch_tsdf_mesh_plan(const gsr_tsdf_grid& g, const float* wsum, const float* dsum, float min_weight, void* scratch, long long totals[2],
                                     hipStream_t s)
{
	{
		GsrProfScope p(s, "tsdf_mesh_plan");
		const GsrTsdfMesh a = gsr_tsdf_mesh_args(g, wsum, dsum, min_weight, scratch);
		const unsigned blocks = gsr_tsdf_blocks(a.nodes);
		hipLaunchKernelGGL(gsr_tsdf_count_kernel, dim3(blocks), dim3(GSR_TSDF_THREADS), 0, s, a);
		hipLaunchKernelGGL(gsr_tsdf_scan_kernel, dim3(1), dim3(GSR_TSDF_SCAN_THREADS), 0, s, blocks, a.wg, a.totals);
	}
	hipError_t e = hipMemcpyAsync(totals, scratch, 2 * sizeof(long long), hipMemcpyDeviceToHost, s);
	if (e == hipSuccess) e = hipStreamSynchronize(s);
	return e;
}

void gsr_launch_tsdf_mesh_emit(const gsr_tsdf_mesh_plan_t& plan, const float* csum, float* vertices, float* colors, int32_t* faces, hipStream_t s)
{
	GsrProfScope p(s, "tsdf_mesh_emit");
	GsrTsdfMesh a = gsr_tsdf_mesh_args(plan.grid, plan.wsum, plan.dsum, plan.min_weight, plan.scratch);
	a.csum = csum; a.V = (unsigned)plan.V; a.F = (unsigned)plan.F;
	a.vertices = vertices; a.colors = colors; a.faces = (int*)faces;
	const unsigned blocks = gsr_tsdf_blocks(a.nodes);
	hipLaunchKernelGGL(gsr_tsdf_vertex_kernel, dim3(blocks), dim3(GSR_TSDF_THREADS), 0, s, a);
	if (plan.F > 0) hipLaunchKernelGGL(gsr_tsdf_face_kernel, dim3(blocks), dim3(GSR_TSDF_THREADS), 0, s, a);
}
