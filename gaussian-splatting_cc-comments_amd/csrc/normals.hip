// normals.hip -- the two ends of the normal-consistency term (include/gsr_normals.h, the contract): one normal per Gaussian, and
// the normals of a depth map's surface, alone or fused with the loss.  The blend in between is the feature pass (features.hip).
//
// Replaces, per training step, about forty stock-PyTorch passes with their autograd backward: rotation matrix, arg-min gather,
// view transform and sign flip over P Gaussians; unprojection, two shifted differences, cross product, normalise, dot and mean over
// H*W pixels.  Here:
//   per-Gaussian: one elementwise kernel forward, one backward (28 B read + 12 B written per Gaussian forward);
//   depth normals forward: one elementwise kernel, the four neighbours read straight from global memory (the cache serves the re-reads);
//   backward / loss: ONE kernel per 64x16 tile.  A pixel's depth enters the normals of its four axis neighbours, so the tile's
//             depths go to LDS with a 2-pixel halo, every centre of the tile and its 1-pixel ring evaluates its normal, the
//             upstream gradient (dL/dout, or -a N / (H W) for the loss) and from them the four scalars it owes its neighbours'
//             depths, leaves them in LDS, and after a barrier every pixel gathers the four scalars addressed to it: no atomics.  The
//             loss variant also writes dL/dnormal_map for the tile's own pixels and one partial sum of a <N, n_d> per workgroup;
//   finalize: one workgroup folds the partial sums in a fixed order (double), as loss.hip's.
// All arithmetic fp32; HBM-bound (loss: 20-24 B read, 16 B written per pixel).
#include "gsr_internal.h"
#include "gsr_depth_key.h"   // gsr_sync()
#include "../../include/gsr_normals.h"

#define GSR_NRM_TX 64
#define GSR_NRM_TY 16
#define GSR_NRM_THREADS 256                  // one column and four rows of the tile per thread in the gather
#define GSR_NRM_ZX (GSR_NRM_TX + 4)          // depths with the 2-pixel halo
#define GSR_NRM_ZY (GSR_NRM_TY + 4)
#define GSR_NRM_CX (GSR_NRM_TX + 2)          // centres with the 1-pixel ring
#define GSR_NRM_CY (GSR_NRM_TY + 2)
static_assert(GSR_NRM_THREADS == 64 * (GSR_NRM_TY / 4), "the gather maps one column and four rows to a thread");

// ---- per-Gaussian normals --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int gsr_min_axis(const float* __restrict__ s)
{
	int k = 0;
	float m = s[0];
	if (s[1] < m) { m = s[1]; k = 1; }
	if (s[2] < m) k = 2;
	return k;
}

// column k of the rotation matrix of the unit quaternion (w, x, y, z) (gsr_model.build_rotation)
__device__ __forceinline__ GsrVec3 gsr_rot_column(int k, float w, float x, float y, float z)
{
	GsrVec3 n;
	if (k == 0) { n.x = 1.f - 2.f * (y * y + z * z); n.y = 2.f * (x * y + w * z); n.z = 2.f * (x * z - w * y); }
	else if (k == 1) { n.x = 2.f * (x * y - w * z); n.y = 1.f - 2.f * (x * x + z * z); n.z = 2.f * (y * z + w * x); }
	else { n.x = 2.f * (x * z + w * y); n.y = 2.f * (y * z - w * x); n.z = 1.f - 2.f * (x * x + y * y); }
	return n;
}

// what both directions share: k, the unit quaternion, |q|, the world normal before the flip and the facing sign
struct GsrNormalOf { int k; float w, x, y, z, len; GsrVec3 nw, nv; float sign; };

__device__ __forceinline__ GsrNormalOf gsr_normal_of(int g, const float* __restrict__ scales, const float* __restrict__ rotations,
                                                     const float* __restrict__ means3D, const float* __restrict__ vm)
{
	GsrNormalOf o;
	const float s[3] = {scales[3 * (size_t)g], scales[3 * (size_t)g + 1], scales[3 * (size_t)g + 2]};
	const float4 q = ((const float4*)rotations)[g];
	const GsrVec3 m = {means3D[3 * (size_t)g], means3D[3 * (size_t)g + 1], means3D[3 * (size_t)g + 2]};
	o.k = gsr_min_axis(s);
	o.len = sqrtf((q.x * q.x + q.y * q.y) + (q.z * q.z + q.w * q.w));
	const float inv = o.len > 0.f ? 1.f / o.len : 0.f;
	o.w = q.x * inv; o.x = q.y * inv; o.y = q.z * inv; o.z = q.w * inv;
	o.nw = gsr_rot_column(o.k, o.w, o.x, o.y, o.z);
	if (!(o.len > 0.f)) o.nw.x = o.nw.y = o.nw.z = 0.f;   // the zero quaternion: no normal (its matrix would be the identity)
	const GsrVec3 t = gsr_transform_point_4x3(m, vm);
	o.nv.x = vm[0] * o.nw.x + vm[4] * o.nw.y + vm[8] * o.nw.z;
	o.nv.y = vm[1] * o.nw.x + vm[5] * o.nw.y + vm[9] * o.nw.z;
	o.nv.z = vm[2] * o.nw.x + vm[6] * o.nw.y + vm[10] * o.nw.z;
	o.sign = (o.nv.x * t.x + o.nv.y * t.y + o.nv.z * t.z) > 0.f ? -1.f : 1.f;
	return o;
}

__global__ void __launch_bounds__(256) gsr_gaussian_normals_kernel(int P, const float* __restrict__ scales, const float* __restrict__ rotations,
                                                                   const float* __restrict__ means3D, const float* __restrict__ vm, int world,
                                                                   float* __restrict__ out)
{
	const int g = blockIdx.x * 256 + threadIdx.x;
	if (g >= P) return;
	const GsrNormalOf o = gsr_normal_of(g, scales, rotations, means3D, vm);
	const GsrVec3 n = world ? o.nw : o.nv;
	out[3 * (size_t)g] = o.sign * n.x;
	out[3 * (size_t)g + 1] = o.sign * n.y;
	out[3 * (size_t)g + 2] = o.sign * n.z;
}

__global__ void __launch_bounds__(256) gsr_gaussian_normals_backward_kernel(int P, const float* __restrict__ scales, const float* __restrict__ rotations,
                                                                            const float* __restrict__ means3D, const float* __restrict__ vm, int world,
                                                                            const float* __restrict__ dL_dout, float* __restrict__ dL_drot)
{
	const int g = blockIdx.x * 256 + threadIdx.x;
	if (g >= P) return;
	const GsrNormalOf o = gsr_normal_of(g, scales, rotations, means3D, vm);
	const float g0 = dL_dout[3 * (size_t)g], g1 = dL_dout[3 * (size_t)g + 1], g2 = dL_dout[3 * (size_t)g + 2];
	// dL/dn_w: the flip, and for the view-space output the transpose of the rotation part of the view transform
	float ax, ay, az;
	if (world) { ax = g0; ay = g1; az = g2; }
	else {
		ax = vm[0] * g0 + vm[1] * g1 + vm[2] * g2;
		ay = vm[4] * g0 + vm[5] * g1 + vm[6] * g2;
		az = vm[8] * g0 + vm[9] * g1 + vm[10] * g2;
	}
	ax *= o.sign; ay *= o.sign; az *= o.sign;
	// dL/d(unit quaternion): the derivatives of gsr_rot_column's three expressions
	const float w = o.w, x = o.x, y = o.y, z = o.z;
	float dw, dx, dy, dz;
	if (o.k == 0) {
		dw = 2.f * (z * ay - y * az);
		dx = 2.f * (y * ay + z * az);
		dy = -4.f * y * ax + 2.f * (x * ay - w * az);
		dz = -4.f * z * ax + 2.f * (w * ay + x * az);
	} else if (o.k == 1) {
		dw = 2.f * (x * az - z * ax);
		dx = -4.f * x * ay + 2.f * (y * ax + w * az);
		dy = 2.f * (x * ax + z * az);
		dz = -4.f * z * ay + 2.f * (y * az - w * ax);
	} else {
		dw = 2.f * (y * ax - x * ay);
		dx = -4.f * x * az + 2.f * (z * ax - w * ay);
		dy = -4.f * y * az + 2.f * (w * ax + z * ay);
		dz = 2.f * (x * ax + y * ay);
	}
	// through q / |q|: (d - qn (qn . d)) / |q|
	float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
	if (o.len > 0.f) {
		const float dot = w * dw + x * dx + y * dy + z * dz, inv = 1.f / o.len;
		r = make_float4((dw - w * dot) * inv, (dx - x * dot) * inv, (dy - y * dot) * inv, (dz - z * dot) * inv);
	}
	((float4*)dL_drot)[g] = r;
}

void gsr_launch_gaussian_normals(int P, const float* scales, const float* rotations, const float* means3D, const float* viewmatrix, int world,
                                 float* out, hipStream_t s)
{
	GsrProfScope p(s, "gaussian_normals");
	hipLaunchKernelGGL(gsr_gaussian_normals_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, scales, rotations, means3D, viewmatrix, world, out);
}

void gsr_launch_gaussian_normals_backward(int P, const float* scales, const float* rotations, const float* means3D, const float* viewmatrix,
                                          int world, const float* dL_dout, float* dL_drot, hipStream_t s)
{
	GsrProfScope p(s, "gaussian_normals_backward");
	hipLaunchKernelGGL(gsr_gaussian_normals_backward_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, scales, rotations, means3D, viewmatrix,
	                   world, dL_dout, dL_drot);
}

// ---- depth normals ---------------------------------------------------------------------------------------------------------------
struct GsrPixelGeom { float tanx, tany, inv_w, inv_h, dx, dy; };

static GsrPixelGeom gsr_pixel_geom(int W, int H, float tanfovx, float tanfovy)
{
	GsrPixelGeom pg = {tanfovx, tanfovy, 1.f / (float)W, 1.f / (float)H, 2.f * tanfovx / (float)W, 2.f * tanfovy / (float)H};
	return pg;
}

__device__ __forceinline__ bool gsr_depth_ok(float z) { return z > 0.f && z <= 3.402823466e38f; }   // finite and positive; NaN fails

// the pixel's normal from its four neighbours' depths (gsr_normals.h); all four must be gsr_depth_ok
struct GsrDepthNormal { float dv, sv, dh, sh, X, Y, len; GsrVec3 n; };

__device__ __forceinline__ GsrDepthNormal gsr_depth_normal(int x, int y, float zu, float zd, float zl, float zr, const GsrPixelGeom& pg)
{
	GsrDepthNormal o;
	o.X = ((float)(2 * x + 1) * pg.inv_w - 1.f) * pg.tanx;
	o.Y = ((float)(2 * y + 1) * pg.inv_h - 1.f) * pg.tany;
	o.dv = zd - zu; o.sv = zd + zu; o.dh = zr - zl; o.sh = zr + zl;
	const float cx = pg.dy * o.sv * o.dh, cy = pg.dx * o.sh * o.dv;
	const float cz = -(o.Y * pg.dx * o.dv * o.sh + o.X * pg.dy * o.sv * o.dh + pg.dx * pg.dy * o.sv * o.sh);
	o.len = sqrtf(cx * cx + cy * cy + cz * cz);
	const float inv = 1.f / fmaxf(o.len, 1e-12f);
	o.n.x = cx * inv; o.n.y = cy * inv; o.n.z = cz * inv;
	return o;
}

// dL/dn of a pixel -> what it owes the depths of its upper, lower, left and right neighbour
__device__ __forceinline__ float4 gsr_depth_normal_adjoint(const GsrDepthNormal& o, float gx, float gy, float gz, const GsrPixelGeom& pg)
{
	// through c / max(|c|, 1e-12)
	float cx, cy, cz;
	if (o.len >= 1e-12f) {
		const float dot = o.n.x * gx + o.n.y * gy + o.n.z * gz, inv = 1.f / o.len;
		cx = (gx - o.n.x * dot) * inv; cy = (gy - o.n.y * dot) * inv; cz = (gz - o.n.z * dot) * inv;
	} else { cx = gx * 1e12f; cy = gy * 1e12f; cz = gz * 1e12f; }
	const float g_dv = pg.dx * o.sh * (cy - o.Y * cz);
	const float g_sv = pg.dy * (cx * o.dh - cz * (o.X * o.dh + pg.dx * o.sh));
	const float g_dh = pg.dy * o.sv * (cx - o.X * cz);
	const float g_sh = pg.dx * (cy * o.dv - cz * (o.Y * o.dv + pg.dy * o.sv));
	return make_float4(g_sv - g_dv, g_sv + g_dv, g_sh - g_dh, g_sh + g_dh);   // up, down, left, right
}

__global__ void __launch_bounds__(256) gsr_depth_normals_kernel(int W, int H, const float* __restrict__ depth, GsrPixelGeom pg,
                                                                float* __restrict__ out)
{
	const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
	if (x >= W || y >= H) return;
	const size_t plane = (size_t)H * W, o = (size_t)y * W + x;
	GsrVec3 n = {0.f, 0.f, 0.f};
	if (x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2) {
		const float zu = depth[o - W], zd = depth[o + W], zl = depth[o - 1], zr = depth[o + 1];
		if (gsr_depth_ok(zu) && gsr_depth_ok(zd) && gsr_depth_ok(zl) && gsr_depth_ok(zr)) n = gsr_depth_normal(x, y, zu, zd, zl, zr, pg).n;
	}
	out[o] = n.x; out[plane + o] = n.y; out[2 * plane + o] = n.z;
}

// LOSS = false: up = dL_dout [3][H][W], the backward of gsr_depth_normals.
// LOSS = true: up = normal_map, the upstream gradient is -a N / (H W); also dL/dnormal_map and the workgroup's sum of a <N, n_d>.
template <bool LOSS>
__global__ void __launch_bounds__(GSR_NRM_THREADS) gsr_depth_normals_tile_kernel(int W, int H, const float* __restrict__ depth,
                                                                                 const float* __restrict__ up, const float* __restrict__ alpha,
                                                                                 GsrPixelGeom pg, float inv_hw, float* __restrict__ dL_dnormal,
                                                                                 float* __restrict__ dL_ddepth, float* __restrict__ partial)
{
	__shared__ float sz[GSR_NRM_ZY * GSR_NRM_ZX];
	__shared__ float4 sg[GSR_NRM_CY * GSR_NRM_CX];   // what each centre owes its upper, lower, left and right neighbour's depth
	__shared__ float wsum[GSR_NRM_THREADS / 64];
	const size_t plane = (size_t)H * W;
	const int x0 = blockIdx.x * GSR_NRM_TX, y0 = blockIdx.y * GSR_NRM_TY;
	// depths with the 2-pixel halo; outside the image 0, which is no valid depth: a centre that is not interior has such a neighbour
	for (int i = threadIdx.x; i < GSR_NRM_ZY * GSR_NRM_ZX; i += GSR_NRM_THREADS) {
		const int gy = y0 - 2 + i / GSR_NRM_ZX, gx = x0 - 2 + i % GSR_NRM_ZX;
		const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
		sz[i] = in ? depth[(size_t)gy * W + gx] : 0.f;
	}
	gsr_sync();
	float sum = 0.f;
	for (int i = threadIdx.x; i < GSR_NRM_CY * GSR_NRM_CX; i += GSR_NRM_THREADS) {
		const int cy = i / GSR_NRM_CX, cx = i % GSR_NRM_CX;
		const int gy = y0 - 1 + cy, gx = x0 - 1 + cx;
		const float* z = sz + (cy + 1) * GSR_NRM_ZX + cx + 1;
		const float zu = z[-GSR_NRM_ZX], zd = z[GSR_NRM_ZX], zl = z[-1], zr = z[1];
		const bool ok = gsr_depth_ok(zu) && gsr_depth_ok(zd) && gsr_depth_ok(zl) && gsr_depth_ok(zr);   // implies an interior pixel of the image
		const bool own = cy >= 1 && cy <= GSR_NRM_TY && cx >= 1 && cx <= GSR_NRM_TX && gy < H && gx < W;   // one of the tile's own pixels
		float4 owes = make_float4(0.f, 0.f, 0.f, 0.f);
		GsrVec3 dn = {0.f, 0.f, 0.f};
		if (ok) {
			const size_t o = (size_t)gy * W + gx;
			const GsrDepthNormal nd = gsr_depth_normal(gx, gy, zu, zd, zl, zr, pg);
			float ux = up[o], uy = up[plane + o], uz = up[2 * plane + o];
			if (LOSS) {
				const float a = alpha ? alpha[o] : 1.f;
				if (own) sum += a * (ux * nd.n.x + uy * nd.n.y + uz * nd.n.z);
				const float f = -(a * inv_hw);
				dn.x = f * nd.n.x; dn.y = f * nd.n.y; dn.z = f * nd.n.z;
				ux *= f; uy *= f; uz *= f;
			}
			owes = gsr_depth_normal_adjoint(nd, ux, uy, uz, pg);
		}
		sg[i] = owes;
		if (LOSS && own && dL_dnormal) {
			const size_t o = (size_t)gy * W + gx;
			dL_dnormal[o] = dn.x; dL_dnormal[plane + o] = dn.y; dL_dnormal[2 * plane + o] = dn.z;
		}
	}
	gsr_sync();
	if (dL_ddepth) {
		const int lx = threadIdx.x & 63, ly0 = (threadIdx.x >> 6) * 4, gx = x0 + lx;
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const int gy = y0 + ly0 + j;
			if (gy >= H || gx >= W) continue;
			const float4* c = sg + (ly0 + j + 1) * GSR_NRM_CX + lx + 1;
			// the centre above owes its lower neighbour, the one below its upper, the one to the left its right, the one to the right its left
			dL_ddepth[(size_t)gy * W + gx] = ((c[-GSR_NRM_CX].y + c[GSR_NRM_CX].x) + c[-1].w) + c[1].z;
		}
	}
	if (LOSS) {
		// fixed-order workgroup reduction -> one partial per tile (deterministic loss value)
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
		if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sum;
		gsr_sync();
		if (threadIdx.x == 0) {
			float t = 0.f;
#pragma unroll
			for (int w = 0; w < GSR_NRM_THREADS / 64; w++) t += wsum[w];
			partial[blockIdx.y * gridDim.x + blockIdx.x] = t;
		}
	}
}

__global__ void __launch_bounds__(256) gsr_normal_loss_finalize_kernel(const float* __restrict__ partial, int n, int H, int W,
                                                                       float* __restrict__ vals)
{
	__shared__ double sl[256];
	double t = 0;
	for (int i = threadIdx.x; i < n; i += 256) t += partial[i];
	sl[threadIdx.x] = t;
	gsr_sync();
	for (int off = 128; off > 0; off >>= 1) {
		if ((int)threadIdx.x < off) sl[threadIdx.x] += sl[threadIdx.x + off];
		gsr_sync();
	}
	if (threadIdx.x == 0) vals[0] = (float)(1.0 - sl[0] / ((double)H * W));
}

static dim3 gsr_normals_grid(int W, int H) { return dim3((W + GSR_NRM_TX - 1) / GSR_NRM_TX, (H + GSR_NRM_TY - 1) / GSR_NRM_TY); }

size_t gsr_normals_scratch_size(int W, int H)
{
	const dim3 g = gsr_normals_grid(W, H);
	return gsr_align_up((size_t)g.x * g.y * sizeof(float));
}

void gsr_launch_depth_normals(int W, int H, const float* depth, float tanfovx, float tanfovy, float* out, hipStream_t s)
{
	GsrProfScope p(s, "depth_normals");
	hipLaunchKernelGGL(gsr_depth_normals_kernel, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, s, W, H, depth,
	                   gsr_pixel_geom(W, H, tanfovx, tanfovy), out);
}

void gsr_launch_depth_normals_backward(int W, int H, const float* depth, float tanfovx, float tanfovy, const float* dL_dout, float* dL_ddepth,
                                       hipStream_t s)
{
	GsrProfScope p(s, "depth_normals_backward");
	hipLaunchKernelGGL(gsr_depth_normals_tile_kernel<false>, gsr_normals_grid(W, H), dim3(GSR_NRM_THREADS), 0, s, W, H, depth, dL_dout,
	                   (const float*)nullptr, gsr_pixel_geom(W, H, tanfovx, tanfovy), 0.f, (float*)nullptr, dL_ddepth, (float*)nullptr);
}

void gsr_launch_normal_consistency_loss(int W, int H, const float* normal_map, const float* depth, const float* alpha, float tanfovx,
                                        float tanfovy, float* vals, float* dL_dnormal, float* dL_ddepth, void* scratch, hipStream_t s)
{
	GsrProfScope p(s, "normal_consistency_loss");
	const dim3 grid = gsr_normals_grid(W, H);
	float* partial = (float*)scratch;
	hipLaunchKernelGGL(gsr_depth_normals_tile_kernel<true>, grid, dim3(GSR_NRM_THREADS), 0, s, W, H, depth, normal_map, alpha,
	                   gsr_pixel_geom(W, H, tanfovx, tanfovy), 1.0f / ((float)H * (float)W), dL_dnormal, dL_ddepth, partial);
	hipLaunchKernelGGL(gsr_normal_loss_finalize_kernel, dim3(1), dim3(256), 0, s, partial, (int)(grid.x * grid.y), H, W, vals);
}
