// rigidity.hip -- the neighbour-rigidity losses of Dynamic 3D Gaussians (rigid, rotation, isometry) over a K-NN table, value and
// gradients of the weighted total in one pass over the edges (include/gsr_rigidity.h).
//
//   rel     one thread per point: rel_i = (r_i / |r_i|) (x) p_i into scratch.  Both ends of an edge read the same stored bits.
//   pass A  GSR_RIG_LANES lanes per point.  The lanes of a point share q, rel and R and take the edges k = lane, lane + LANES, ...,
//           so that a load instruction of the group reads consecutive entries of a (P, K, .) row.  Each lane adds its edges in
//           ascending k; the lanes are then added by a fixed xor tree.  A valid edge stores its neighbour-side row (dL/dx_j, 3 floats;
//           dL/drel_j, 4 floats) with plain stores; the first lane folds dL/dR to the quaternion and stores the centre-side row.
//   pass B  one thread per point: the incoming edge rows over edges[offsets[j] .. offsets[j + 1]) in ascending edge id, then the
//           centre-side row, then dL/drel_j through (x) p_j and the normalisation.  One owner per output row, one store each.
//   fold    the per-workgroup value partials in double, a fixed order, divided by N_e = offsets[P].
// No atomics; every sum has a fixed order, so every output has the same bits in every run.
// Quaternions are (w, x, y, z) in the members .x .y .z .w of a float4.
#include "gsr_internal.h"
#include "gsr_depth_key.h"   // gsr_sync()

#ifndef GSR_RIG_LANES
#define GSR_RIG_LANES 8      // lanes per point in pass A; 1, 2, 4, 8, 16 measured
#endif
#define GSR_RIG_THREADS 256
#define GSR_RIG_POINTS (GSR_RIG_THREADS / GSR_RIG_LANES)   // points per workgroup in pass A
#define GSR_RIG_EPS 1e-20f

__device__ __forceinline__ float4 gsr_rig_quat_mult(float4 a, float4 b)
{
	return make_float4(a.x * b.x - a.y * b.y - a.z * b.z - a.w * b.w,
	                   a.x * b.y + a.y * b.x + a.z * b.w - a.w * b.z,
	                   a.x * b.z - a.y * b.w + a.z * b.x + a.w * b.y,
	                   a.x * b.w + a.y * b.z - a.z * b.y + a.w * b.x);
}

__device__ __forceinline__ float4 gsr_rig_load4(const float* __restrict__ p, size_t i)   // the caller's rows: 4-byte alignment only
{
	return make_float4(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]);
}

__global__ void __launch_bounds__(256) gsr_rig_rel_kernel(int P, const float* __restrict__ rotation, const float* __restrict__ prev_inv_rot,
                                                          float4* __restrict__ rel)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= P) return;
	const float4 r = gsr_rig_load4(rotation, i), p = gsr_rig_load4(prev_inv_rot, i);
	const float n = sqrtf(r.x * r.x + r.y * r.y + r.z * r.z + r.w * r.w);
	rel[i] = gsr_rig_quat_mult(make_float4(r.x / n, r.y / n, r.z / n, r.w / n), p);
}

// GRAD = false: values only, nothing but `partial` is written.  edge_x / centre_x and edge_rel / centre_rel are NULL in pairs where
// that gradient is not wanted.
template <bool GRAD>
__global__ void __launch_bounds__(GSR_RIG_THREADS) gsr_rig_edges_kernel(int P, int K, const float* __restrict__ xyz, const float4* __restrict__ rel,
                                                                        const int* __restrict__ idx, const float* __restrict__ prev_offset,
                                                                        const float* __restrict__ prev_dist, const float* __restrict__ weight,
                                                                        const int* __restrict__ offsets, float w_rigid, float w_rot, float w_iso,
                                                                        float4* __restrict__ centre_rel, float* __restrict__ centre_x,
                                                                        float4* __restrict__ edge_rel, float* __restrict__ edge_x, float* __restrict__ partial)
{
	__shared__ float wsum[GSR_RIG_THREADS / 64][3];
	const int i = blockIdx.x * GSR_RIG_POINTS + (int)(threadIdx.x / GSR_RIG_LANES);
	const int lane = (int)(threadIdx.x % GSR_RIG_LANES);
	const bool active = i < P;
	float vr = 0.f, vo = 0.f, vi = 0.f;                 // value partials
	float ax = 0.f, ay = 0.f, az = 0.f;                 // dL/dx_i
	float4 ar = make_float4(0.f, 0.f, 0.f, 0.f);        // dL/drel_i, rotation term
	float G[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};   // G[b][a] = dL/dR[b][a]
	float4 v = make_float4(1.f, 0.f, 0.f, 0.f);
	float nr = 1.f;
	if (active) {
		const int ne = offsets[P];
		const double inv = ne > 0 ? 1.0 / (double)ne : 0.0;
		const float cr = (float)((double)w_rigid * inv), co = (float)((double)w_rot * inv), ci = (float)((double)w_iso * inv);
		const float xi = xyz[3 * (size_t)i], yi = xyz[3 * (size_t)i + 1], zi = xyz[3 * (size_t)i + 2];
		const float4 ri = rel[i];
		nr = sqrtf(ri.x * ri.x + ri.y * ri.y + ri.z * ri.z + ri.w * ri.w);
		v = make_float4(ri.x / nr, ri.y / nr, ri.z / nr, ri.w / nr);
		const float r = v.x, x = v.y, y = v.z, z = v.w;
		const float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - r * z), R02 = 2.f * (x * z + r * y);
		const float R10 = 2.f * (x * y + r * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - r * x);
		const float R20 = 2.f * (x * z - r * y), R21 = 2.f * (y * z + r * x), R22 = 1.f - 2.f * (x * x + y * y);
		for (int k = lane; k < K; k += GSR_RIG_LANES) {
			const size_t e = (size_t)i * (size_t)K + (size_t)k;
			const int j = idx[e];
			if ((unsigned)j >= (unsigned)P) continue;   // -1: no edge (and nothing of this place is read); out of range counts as none
			const float w = weight[e], d = prev_dist[e];
			const float ox = prev_offset[3 * e], oy = prev_offset[3 * e + 1], oz = prev_offset[3 * e + 2];
			const float4 rj = rel[j];
			const float cx = xyz[3 * (size_t)j] - xi, cy = xyz[3 * (size_t)j + 1] - yi, cz = xyz[3 * (size_t)j + 2] - zi;
			// rigid: u = R^T c - o
			const float ux = R00 * cx + R10 * cy + R20 * cz - ox;
			const float uy = R01 * cx + R11 * cy + R21 * cz - oy;
			const float uz = R02 * cx + R12 * cy + R22 * cz - oz;
			const float sr = sqrtf(w * (ux * ux + uy * uy + uz * uz) + GSR_RIG_EPS);
			// rotation: m = rel_j - rel_i
			const float mw = rj.x - ri.x, mx = rj.y - ri.y, my = rj.z - ri.z, mz = rj.w - ri.w;
			const float so = sqrtf(w * (mw * mw + mx * mx + my * my + mz * mz) + GSR_RIG_EPS);
			// isometry
			const float len = sqrtf(cx * cx + cy * cy + cz * cz + GSR_RIG_EPS);
			const float t = len - d;
			const float si = sqrtf(w * (t * t) + GSR_RIG_EPS);
			vr += sr; vo += so; vi += si;
			if (GRAD) {
				const float fr = cr * w / sr, fo = co * w / so, fl = ci * w * t / si / len;
				const float gux = fr * ux, guy = fr * uy, guz = fr * uz;
				const float gcx = R00 * gux + R01 * guy + R02 * guz + fl * cx;   // dL/dc = R gu + (dL/dlen / len) c
				const float gcy = R10 * gux + R11 * guy + R12 * guz + fl * cy;
				const float gcz = R20 * gux + R21 * guy + R22 * guz + fl * cz;
				const float4 gm = make_float4(fo * mw, fo * mx, fo * my, fo * mz);
				ax -= gcx; ay -= gcy; az -= gcz;
				ar.x -= gm.x; ar.y -= gm.y; ar.z -= gm.z; ar.w -= gm.w;
				G[0][0] += cx * gux; G[0][1] += cx * guy; G[0][2] += cx * guz;
				G[1][0] += cy * gux; G[1][1] += cy * guy; G[1][2] += cy * guz;
				G[2][0] += cz * gux; G[2][1] += cz * guy; G[2][2] += cz * guz;
				if (edge_x) { edge_x[3 * e] = gcx; edge_x[3 * e + 1] = gcy; edge_x[3 * e + 2] = gcz; }
				if (edge_rel) edge_rel[e] = gm;
			}
		}
	}
	if (GRAD) {
		// the lanes of a point, a fixed xor tree (every lane of the wave takes part; an idle group adds zeros)
#pragma unroll
		for (int off = GSR_RIG_LANES / 2; off > 0; off >>= 1) {
			ax += __shfl_xor(ax, off, 64); ay += __shfl_xor(ay, off, 64); az += __shfl_xor(az, off, 64);
			ar.x += __shfl_xor(ar.x, off, 64); ar.y += __shfl_xor(ar.y, off, 64); ar.z += __shfl_xor(ar.z, off, 64); ar.w += __shfl_xor(ar.w, off, 64);
#pragma unroll
			for (int b = 0; b < 3; b++)
#pragma unroll
				for (int a = 0; a < 3; a++) G[b][a] += __shfl_xor(G[b][a], off, 64);
		}
		if (active && lane == 0) {
			if (centre_x) { centre_x[3 * (size_t)i] = ax; centre_x[3 * (size_t)i + 1] = ay; centre_x[3 * (size_t)i + 2] = az; }
			if (centre_rel) {
				// dL/dR -> dL/dv for R = R(v), then through v = rel / |rel|
				const float r = v.x, x = v.y, y = v.z, z = v.w;
				const float gr = 2.f * (-z * G[0][1] + y * G[0][2] + z * G[1][0] - x * G[1][2] - y * G[2][0] + x * G[2][1]);
				const float gx = 2.f * (y * G[0][1] + z * G[0][2] + y * G[1][0] - 2.f * x * G[1][1] - r * G[1][2] + z * G[2][0] + r * G[2][1] - 2.f * x * G[2][2]);
				const float gy = 2.f * (-2.f * y * G[0][0] + x * G[0][1] + r * G[0][2] + x * G[1][0] + z * G[1][2] - r * G[2][0] + z * G[2][1] - 2.f * y * G[2][2]);
				const float gz = 2.f * (-2.f * z * G[0][0] - r * G[0][1] + x * G[0][2] + r * G[1][0] - 2.f * z * G[1][1] + y * G[1][2] + x * G[2][0] + y * G[2][1]);
				const float dot = r * gr + x * gx + y * gy + z * gz;
				centre_rel[i] = make_float4(ar.x + (gr - r * dot) / nr, ar.y + (gx - x * dot) / nr, ar.z + (gy - y * dot) / nr, ar.w + (gz - z * dot) / nr);
			}
		}
	}
	// values: the wave as a tree, then the four waves
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		vr += __shfl_down(vr, off, 64); vo += __shfl_down(vo, off, 64); vi += __shfl_down(vi, off, 64);
	}
	if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6][0] = vr; wsum[threadIdx.x >> 6][1] = vo; wsum[threadIdx.x >> 6][2] = vi; }
	gsr_sync();
	if (threadIdx.x < 3)
		partial[3 * (size_t)blockIdx.x + threadIdx.x] = (wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + (wsum[2][threadIdx.x] + wsum[3][threadIdx.x]);
}

// Pass B.  The loads of four edges are issued together; the additions keep the edge order.
template <bool WX, bool WR>
__global__ void __launch_bounds__(256) gsr_rig_gather_kernel(int P, const int* __restrict__ offsets, const int* __restrict__ edges,
                                                             const float4* __restrict__ centre_rel, const float* __restrict__ centre_x,
                                                             const float4* __restrict__ edge_rel, const float* __restrict__ edge_x,
                                                             const float* __restrict__ rotation, const float* __restrict__ prev_inv_rot,
                                                             float* __restrict__ grad_xyz, float* __restrict__ grad_rot)
{
	const int j = blockIdx.x * 256 + threadIdx.x;
	if (j >= P) return;
	const int lo = offsets[j], hi = offsets[j + 1];
	float ax = 0.f, ay = 0.f, az = 0.f;
	float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
	int n = lo;
	for (; n + 4 <= hi; n += 4) {
		size_t e[4];
		float px[4][3];
		float4 pr[4];
#pragma unroll
		for (int u = 0; u < 4; u++) e[u] = (size_t)edges[n + u];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			if (WX) { px[u][0] = edge_x[3 * e[u]]; px[u][1] = edge_x[3 * e[u] + 1]; px[u][2] = edge_x[3 * e[u] + 2]; }
			if (WR) pr[u] = edge_rel[e[u]];
		}
#pragma unroll
		for (int u = 0; u < 4; u++) {
			if (WX) { ax += px[u][0]; ay += px[u][1]; az += px[u][2]; }
			if (WR) { g.x += pr[u].x; g.y += pr[u].y; g.z += pr[u].z; g.w += pr[u].w; }
		}
	}
	for (; n < hi; n++) {
		const size_t e = (size_t)edges[n];
		if (WX) { ax += edge_x[3 * e]; ay += edge_x[3 * e + 1]; az += edge_x[3 * e + 2]; }
		if (WR) { const float4 p = edge_rel[e]; g.x += p.x; g.y += p.y; g.z += p.z; g.w += p.w; }
	}
	if (WX) {
		grad_xyz[3 * (size_t)j] = ax + centre_x[3 * (size_t)j];
		grad_xyz[3 * (size_t)j + 1] = ay + centre_x[3 * (size_t)j + 1];
		grad_xyz[3 * (size_t)j + 2] = az + centre_x[3 * (size_t)j + 2];
	}
	if (WR) {
		const float4 c = centre_rel[j];
		g.x += c.x; g.y += c.y; g.z += c.z; g.w += c.w;
		// rel = q (x) p is linear in q: dL/dq = dL/drel (x) conj(p); then q = r / |r|
		const float4 r = gsr_rig_load4(rotation, j), p = gsr_rig_load4(prev_inv_rot, j);
		const float4 gq = gsr_rig_quat_mult(g, make_float4(p.x, -p.y, -p.z, -p.w));
		const float nq = sqrtf(r.x * r.x + r.y * r.y + r.z * r.z + r.w * r.w);
		const float4 q = make_float4(r.x / nq, r.y / nq, r.z / nq, r.w / nq);
		const float dot = q.x * gq.x + q.y * gq.y + q.z * gq.z + q.w * gq.w;
		grad_rot[4 * (size_t)j] = (gq.x - q.x * dot) / nq;
		grad_rot[4 * (size_t)j + 1] = (gq.y - q.y * dot) / nq;
		grad_rot[4 * (size_t)j + 2] = (gq.z - q.z * dot) / nq;
		grad_rot[4 * (size_t)j + 3] = (gq.w - q.w * dot) / nq;
	}
}

// values = {total, rigid, rot, iso}: the workgroups' partials in double (thread t takes t, t + 256, ...; the wave and the four waves as
// trees), each divided by N_e; the total from the unrounded terms, rounded once.  n = 0: zeros.
__global__ void __launch_bounds__(256) gsr_rig_fold_kernel(const float* __restrict__ partial, int n, const int* __restrict__ offsets, int P, double w_rigid,
                                                           double w_rot, double w_iso, float* __restrict__ values)
{
	__shared__ double sw[4][3];
	double v[3] = {0.0, 0.0, 0.0};
	for (int i = threadIdx.x; i < n; i += 256) {
		v[0] += (double)partial[3 * (size_t)i]; v[1] += (double)partial[3 * (size_t)i + 1]; v[2] += (double)partial[3 * (size_t)i + 2];
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		v[0] += __shfl_down(v[0], off, 64); v[1] += __shfl_down(v[1], off, 64); v[2] += __shfl_down(v[2], off, 64);
	}
	if ((threadIdx.x & 63) == 0) { sw[threadIdx.x >> 6][0] = v[0]; sw[threadIdx.x >> 6][1] = v[1]; sw[threadIdx.x >> 6][2] = v[2]; }
	gsr_sync();
	if (threadIdx.x == 0) {
		const int ne = n > 0 ? offsets[P] : 0;
		const double inv = ne > 0 ? 1.0 / (double)ne : 0.0;
		double t[3];
#pragma unroll
		for (int c = 0; c < 3; c++) t[c] = ne > 0 ? ((sw[0][c] + sw[1][c]) + (sw[2][c] + sw[3][c])) * inv : 0.0;
		values[0] = (float)(w_rigid * t[0] + w_rot * t[1] + w_iso * t[2]);
		values[1] = (float)t[0]; values[2] = (float)t[1]; values[3] = (float)t[2];
	}
}

// ---- host side ----
static long long gsr_rig_blocks(int P) { return ((long long)P + GSR_RIG_POINTS - 1) / GSR_RIG_POINTS; }

struct GsrRigScratch { float4 *rel, *centre_rel, *edge_rel; float *centre_x, *edge_x, *partial; size_t total; };

static GsrRigScratch gsr_rig_carve(void* base, int P, int K)
{
	size_t off = 0;
	auto take = [&](size_t bytes) { void* p = (char*)base + off; off += gsr_align_up(bytes); return p; };
	const size_t E = (size_t)P * (size_t)K;
	GsrRigScratch r;
	r.rel = (float4*)take(16 * (size_t)P);
	r.partial = (float*)take(12 * (size_t)gsr_rig_blocks(P));
	r.centre_rel = (float4*)take(16 * (size_t)P);
	r.centre_x = (float*)take(12 * (size_t)P);
	r.edge_rel = (float4*)take(16 * E);
	r.edge_x = (float*)take(12 * E);
	r.total = off;
	return r;
}

size_t gsr_rigidity_scratch_size(int P, int K) { return (P > 0 && K > 0) ? gsr_rig_carve(nullptr, P, K).total : 0; }

void gsr_launch_rigidity_zero(int P, float* values, float* grad_xyz, float* grad_rot, hipStream_t s)
{
	GsrProfScope p(s, "rigidity_fold");
	hipLaunchKernelGGL(gsr_rig_fold_kernel, dim3(1), dim3(256), 0, s, (const float*)nullptr, 0, (const int*)nullptr, 0, 0.0, 0.0, 0.0, values);
	if (P > 0 && grad_xyz) (void)hipMemsetAsync(grad_xyz, 0, 12 * (size_t)P, s);
	if (P > 0 && grad_rot) (void)hipMemsetAsync(grad_rot, 0, 16 * (size_t)P, s);
}

void gsr_launch_rigidity_loss(int P, int K, const float* xyz, const float* rotation, const int* idx, const float* prev_offset, const float* prev_dist,
                              const float* weight, const float* prev_inv_rot, const int* offsets, const int* edges, float w_rigid, float w_rot, float w_iso,
                              float* values, float* grad_xyz, float* grad_rot, void* scratch, hipStream_t s)
{
	const GsrRigScratch r = gsr_rig_carve(scratch, P, K);
	const unsigned blocks = (unsigned)gsr_rig_blocks(P), rows = (unsigned)(((long long)P + 255) / 256);
	const bool grad = grad_xyz || grad_rot;
	{
		GsrProfScope p(s, "rigidity_edges");
		hipLaunchKernelGGL(gsr_rig_rel_kernel, dim3(rows), dim3(256), 0, s, P, rotation, prev_inv_rot, r.rel);
		if (grad)
			hipLaunchKernelGGL(gsr_rig_edges_kernel<true>, dim3(blocks), dim3(GSR_RIG_THREADS), 0, s, P, K, xyz, (const float4*)r.rel, idx, prev_offset, prev_dist,
			                   weight, offsets, w_rigid, w_rot, w_iso, grad_rot ? r.centre_rel : nullptr, grad_xyz ? r.centre_x : nullptr,
			                   grad_rot ? r.edge_rel : nullptr, grad_xyz ? r.edge_x : nullptr, r.partial);
		else
			hipLaunchKernelGGL(gsr_rig_edges_kernel<false>, dim3(blocks), dim3(GSR_RIG_THREADS), 0, s, P, K, xyz, (const float4*)r.rel, idx, prev_offset, prev_dist,
			                   weight, offsets, w_rigid, w_rot, w_iso, (float4*)nullptr, (float*)nullptr, (float4*)nullptr, (float*)nullptr, r.partial);
	}
	GsrProfScope p(s, "rigidity_fold");
	if (grad_xyz && grad_rot)
		hipLaunchKernelGGL((gsr_rig_gather_kernel<true, true>), dim3(rows), dim3(256), 0, s, P, offsets, edges, (const float4*)r.centre_rel, (const float*)r.centre_x,
		                   (const float4*)r.edge_rel, (const float*)r.edge_x, rotation, prev_inv_rot, grad_xyz, grad_rot);
	else if (grad_xyz)
		hipLaunchKernelGGL((gsr_rig_gather_kernel<true, false>), dim3(rows), dim3(256), 0, s, P, offsets, edges, (const float4*)r.centre_rel, (const float*)r.centre_x,
		                   (const float4*)r.edge_rel, (const float*)r.edge_x, rotation, prev_inv_rot, grad_xyz, grad_rot);
	else if (grad_rot)
		hipLaunchKernelGGL((gsr_rig_gather_kernel<false, true>), dim3(rows), dim3(256), 0, s, P, offsets, edges, (const float4*)r.centre_rel, (const float*)r.centre_x,
		                   (const float4*)r.edge_rel, (const float*)r.edge_x, rotation, prev_inv_rot, grad_xyz, grad_rot);
	hipLaunchKernelGGL(gsr_rig_fold_kernel, dim3(1), dim3(256), 0, s, (const float*)r.partial, (int)blocks, offsets, P, (double)w_rigid, (double)w_rot, (double)w_iso,
	                   values);
}
