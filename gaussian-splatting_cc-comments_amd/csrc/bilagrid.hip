// bilagrid.hip -- the per-image bilateral grid of affine colour transforms (include/gsr_bilagrid.h): slice, its backward, total variation.
//
//   slice / dL_dimg: one streaming kernel over the image (a template on the direction), a 64x32 tile per workgroup, eight pixels of one
//             column per thread.  The node window of the tile -- the grid cells its pixels can fall in, all L levels -- is staged in
//             LDS with the twelve channels of a node side by side (three 16-byte reads per corner).  A window that does not fit is
//             staged in passes over its node rows; where not even two node rows fit (more nodes than pixels, or a very long luma
//             axis) the corners come straight from global memory.
//   dL_dgrid: a gather.  One workgroup per spatial node and group of GSR_BG_LC luma levels walks the pixels of the node's support
//             (the four cells around it) row by row, every thread keeps 12 x GSR_BG_LC sums, and they are added lanes first
//             (__shfl_down), then waves in wave order through LDS.  No pixel is added to a node by two workgroups, so there is
//             nothing to fold -- unless the grid has too few nodes to fill the device: then the support is cut into S row segments
//             (blockIdx.y), each writes its row of partial sums to scratch, and a second kernel adds the rows in segment order in
//             double precision.
//   tv:       elementwise over all grids with the six neighbours read through the cache; value partials per workgroup in a fixed
//             order, one workgroup folds them in double precision (the order of gsr_loss_ext_finalize_kernel).
// No atomics.  Indices are 32-bit: api.hip refuses sizes beyond that.
#include <algorithm>

#include "gsr_internal.h"
#include "../../include/gsr_bilagrid.h"

#define GSR_BG_TX 64
#define GSR_BG_TY 32
#define GSR_BG_THREADS 256
#define GSR_BG_WAVES (GSR_BG_THREADS / 64)
#define GSR_BG_ROWS (GSR_BG_TY / GSR_BG_WAVES)   // pixels per thread: one column, this many rows
#define GSR_BG_LDS_BYTES (64 * 1024)             // the most a node window may take
// The gather's constants, swept on the MI355X with the default grid at 1980x1080 / 3840x2160 (tools/bilagrid_bench.py over `make variant`
// builds, dL_dgrid alone): 256 / 512 / 1024 threads 0.113 / 0.099 / 0.108 and 0.369 / 0.309 / 0.325 ms; eight levels per workgroup (half
// the reads, 256 workgroups) 0.120 / 0.392 against 0.113 / 0.370; row segments where the grid alone gives 512 workgroups (FILL 2048 / 4096 /
// 8192) 0.166 / 0.177 / 0.173 against 0.115 -- a node's support covers a fraction of the image's rows, so most segments are empty.
#ifndef GSR_BG_LC
#define GSR_BG_LC 4                              // luma levels per gather workgroup
#endif
#ifndef GSR_BG_FILL
#define GSR_BG_FILL 512                          // the gather is cut into row segments below this many workgroups ...
#endif
#ifndef GSR_BG_GATHER_THREADS
#define GSR_BG_GATHER_THREADS 512                // of a gather workgroup: one image row of the support per wave at a time
#endif
#define GSR_BG_GATHER_WAVES (GSR_BG_GATHER_THREADS / 64)

#define GSR_BG_MAX_SEGMENTS 64                   // ... into at most this many
#define GSR_BG_TV_PER_THREAD 4

// cell index and weight of pixel i along one spatial axis: g = (i + 0.5) / size * (n - 1) lies in (0, n - 1).  The operations of the
// definition in its order (a correctly rounded division included), so that a plain fp32 evaluation of it finds the same cell.
__device__ __forceinline__ int gsr_bg_cell(int i, float size, int n, float& t)
{
	const float g = ((float)i + 0.5f) / size * (float)(n - 1);
	const int c = min((int)g, n - 2);
	t = g - (float)c;
	return c;
}

// the same along the luma axis; `inside`: the guidance term of dL_dimg is alive (PyTorch's border rule)
__device__ __forceinline__ int gsr_bg_level(float r, float g, float b, float lm, int L, float& t, bool& inside)
{
	const float luma = __builtin_fmaf(0.114f, b, __builtin_fmaf(0.587f, g, 0.299f * r));
	const float zf = luma * lm;
	inside = zf > 0.f && zf < lm;
	const float gz = fminf(fmaxf(zf, 0.f), lm);   // a NaN becomes 0: the index stays inside the grid whatever the image holds
	const int z = min((int)gz, L - 2);
	t = gz - (float)z;
	return z;
}

// the hat weight of node n for a pixel in cell c with weight t
__device__ __forceinline__ float gsr_bg_hat(int n, int c, float t) { return c == n ? 1.f - t : (c + 1 == n ? t : 0.f); }

struct GsrBgSlice {
	int H, W, L, GH, GW, tiles_x;
	float sx, sy, lm;      // W, H, L - 1 as floats
	int lds_floats;
	const float *grid, *img, *G;
	float* dst;            // out, or dL_dimg
};

struct GsrBgWindow {
	const float* lds;      // [L][nr][nwx][12]: node rows row0 .. row0 + nr - 1, node columns x0 .. x0 + nwx - 1
	const float* grid;
	bool staged;
	int x0, row0, nwx, nr, GH, GW;
	unsigned plane;        // L GH GW
};

template <bool STAGED>
__device__ __forceinline__ void gsr_bg_node(const GsrBgWindow& w, int z, int y, int x, float (&a)[12])
{
	if constexpr (STAGED) {
		const float4* p = (const float4*)(w.lds + ((z * w.nr + (y - w.row0)) * w.nwx + (x - w.x0)) * 12);
		const float4 q0 = p[0], q1 = p[1], q2 = p[2];
		a[0] = q0.x; a[1] = q0.y; a[2] = q0.z; a[3] = q0.w;
		a[4] = q1.x; a[5] = q1.y; a[6] = q1.z; a[7] = q1.w;
		a[8] = q2.x; a[9] = q2.y; a[10] = q2.z; a[11] = q2.w;
	} else {
		const float* p = w.grid + ((unsigned)(z * w.GH + y) * (unsigned)w.GW + (unsigned)x);
#pragma unroll
		for (int ch = 0; ch < 12; ch++) a[ch] = p[(size_t)ch * w.plane];
	}
}

// the twelve channels on luma level z, bilinear in xy
template <bool STAGED>
__device__ __forceinline__ void gsr_bg_bilinear(const GsrBgWindow& w, int z, int cy, int cx, float ty, float tx, float (&A)[12])
{
	float n00[12], n01[12], n10[12], n11[12];
	gsr_bg_node<STAGED>(w, z, cy, cx, n00);
	gsr_bg_node<STAGED>(w, z, cy, cx + 1, n01);
	gsr_bg_node<STAGED>(w, z, cy + 1, cx, n10);
	gsr_bg_node<STAGED>(w, z, cy + 1, cx + 1, n11);
	const float w00 = (1.f - ty) * (1.f - tx), w01 = (1.f - ty) * tx, w10 = ty * (1.f - tx), w11 = ty * tx;
#pragma unroll
	for (int i = 0; i < 12; i++) A[i] = w00 * n00[i] + w01 * n01[i] + w10 * n10[i] + w11 * n11[i];
}

// this thread's pixels (column x, rows yt ..) whose cell row lies in [cy_first, cy_last]: the rows of cells the window holds
template <bool BWD, bool STAGED>
__device__ __forceinline__ void gsr_bg_rows(const GsrBgSlice& a, const GsrBgWindow& w, int x, int yt, int cx, float tx, int cy_first, int cy_last)
{
	const int H = a.H, W = a.W, L = a.L, GH = a.GH;
	const unsigned plane = (unsigned)H * (unsigned)W;
#pragma unroll 1
	for (int j = 0; j < GSR_BG_ROWS; j++) {
		const int y = yt + j;
		if (x >= W || y >= H) continue;
		float ty;
		const int cy = gsr_bg_cell(y, a.sy, GH, ty);
		if (cy < cy_first || cy > cy_last) continue;   // another pass holds this pixel's two node rows
		const unsigned o = (unsigned)y * (unsigned)W + (unsigned)x;
		const float v[4] = {a.img[o], a.img[plane + o], a.img[2 * plane + o], 1.f};
		float tz;
		bool inside;
		const int z = gsr_bg_level(v[0], v[1], v[2], a.lm, L, tz, inside);
		float A0[12], A1[12];
		gsr_bg_bilinear<STAGED>(w, z, cy, cx, ty, tx, A0);
		gsr_bg_bilinear<STAGED>(w, z + 1, cy, cx, ty, tx, A1);
		if constexpr (!BWD) {
#pragma unroll
			for (int c = 0; c < 3; c++) {
				float A[4];
#pragma unroll
				for (int k = 0; k < 4; k++) A[k] = (1.f - tz) * A0[4 * c + k] + tz * A1[4 * c + k];
				a.dst[c * plane + o] = __builtin_fmaf(A[2], v[2], __builtin_fmaf(A[1], v[1], __builtin_fmaf(A[0], v[0], A[3])));
			}
		} else {
			const float G[3] = {a.G[o], a.G[plane + o], a.G[2 * plane + o]};
			float d[3] = {0.f, 0.f, 0.f}, dz = 0.f;   // through the affine map; d (out . G) / d gz
#pragma unroll
			for (int c = 0; c < 3; c++) {
				float s = 0.f;
#pragma unroll
				for (int k = 0; k < 4; k++) {
					if (k < 3) d[k] = __builtin_fmaf((1.f - tz) * A0[4 * c + k] + tz * A1[4 * c + k], G[c], d[k]);
					s = __builtin_fmaf(A1[4 * c + k] - A0[4 * c + k], v[k], s);
				}
				dz = __builtin_fmaf(G[c], s, dz);
			}
			dz = inside ? dz * a.lm : 0.f;
			a.dst[o] = __builtin_fmaf(0.299f, dz, d[0]);
			a.dst[plane + o] = __builtin_fmaf(0.587f, dz, d[1]);
			a.dst[2 * plane + o] = __builtin_fmaf(0.114f, dz, d[2]);
		}
	}
}

template <bool BWD>
__global__ void __launch_bounds__(GSR_BG_THREADS) gsr_bilagrid_pixel_kernel(const GsrBgSlice a)
{
	extern __shared__ __attribute__((aligned(16))) float lds[];
	const int H = a.H, W = a.W, L = a.L, GH = a.GH, GW = a.GW;
	const int px0 = (blockIdx.x % a.tiles_x) * GSR_BG_TX, py0 = (blockIdx.x / a.tiles_x) * GSR_BG_TY;
	const int px1 = min(px0 + GSR_BG_TX, W) - 1, py1 = min(py0 + GSR_BG_TY, H) - 1;
	float t;
	const int cx_lo = gsr_bg_cell(px0, a.sx, GW, t), cx_hi = gsr_bg_cell(px1, a.sx, GW, t);
	const int cy_lo = gsr_bg_cell(py0, a.sy, GH, t), cy_hi = gsr_bg_cell(py1, a.sy, GH, t);
	const int nwx = cx_hi - cx_lo + 2, nwy = cy_hi - cy_lo + 2;   // nodes the tile's pixels touch
	const int per_row = nwx * L * 12;
	int NR = min(nwy, a.lds_floats / per_row);                    // node rows per pass
	GsrBgWindow w;
	w.lds = lds; w.grid = a.grid; w.staged = NR >= 2; w.x0 = cx_lo; w.nwx = nwx; w.GH = GH; w.GW = GW;
	w.plane = (unsigned)L * (unsigned)GH * (unsigned)GW;
	if (!w.staged) NR = nwy;                                      // one pass, the corners from global memory
	const int x = px0 + (threadIdx.x & 63), yt = py0 + (threadIdx.x >> 6) * GSR_BG_ROWS;
	float tx = 0.f;
	const int cx = gsr_bg_cell(min(x, W - 1), a.sx, GW, tx);
	for (int r0 = 0; r0 < nwy - 1; r0 += NR - 1) {
		const int nr = min(NR, nwy - r0);
		w.row0 = cy_lo + r0; w.nr = nr;
		if (w.staged) {
			if (r0 > 0) __syncthreads();   // the previous pass has been read
			const int nodes = L * nr * nwx, rows = nr * nwx;
			for (int i = threadIdx.x; i < 12 * nodes; i += GSR_BG_THREADS) {
				const int ch = i / nodes, n = i - ch * nodes;
				const int z = n / rows, q = n - z * rows;
				const int yy = q / nwx, xx = q - yy * nwx;
				lds[n * 12 + ch] = a.grid[(unsigned)((ch * L + z) * GH + w.row0 + yy) * (unsigned)GW + (unsigned)(cx_lo + xx)];
			}
			__syncthreads();
		}
		if (w.staged) gsr_bg_rows<BWD, true>(a, w, x, yt, cx, tx, cy_lo + r0, cy_lo + r0 + nr - 2);
		else gsr_bg_rows<BWD, false>(a, w, x, yt, cx, tx, cy_lo + r0, cy_lo + r0 + nr - 2);
	}
}

struct GsrBgGather {
	int H, W, L, GH, GW, nch, RS;   // nch: level groups per node; RS: image rows per segment
	float sx, sy, lm;
	const float *img, *G;
	float* dst;                     // dL_dgrid, or the segments' rows in scratch
	unsigned ngrid;                 // 12 L GH GW
};

__global__ void __launch_bounds__(GSR_BG_GATHER_THREADS) gsr_bilagrid_grid_backward_kernel(const GsrBgGather a)
{
	__shared__ float wsum[GSR_BG_GATHER_WAVES][12 * GSR_BG_LC];
	const int H = a.H, W = a.W, L = a.L, GH = a.GH, GW = a.GW;
	const int node = blockIdx.x / a.nch, l0 = (blockIdx.x % a.nch) * GSR_BG_LC, seg = blockIdx.y;
	const int ny = node / GW, nx = node % GW;
	// a superset of the pixels whose cell touches the node: |g - n| < 1 with one pixel to spare on either side; the hat weight
	// decides, and is 0 for the spare ones
	const int x_lo = nx > 0 ? max(0, (int)((long long)W * (nx - 1) / (GW - 1)) - 1) : 0;
	const int x_hi = (int)min((long long)W - 1, ((long long)W * (nx + 1) + GW - 2) / (GW - 1) + 1);
	int y_lo = ny > 0 ? max(0, (int)((long long)H * (ny - 1) / (GH - 1)) - 1) : 0;
	int y_hi = (int)min((long long)H - 1, ((long long)H * (ny + 1) + GH - 2) / (GH - 1) + 1);
	y_lo = max(y_lo, seg * a.RS);
	y_hi = (int)min((long long)y_hi, (long long)seg * a.RS + a.RS - 1);
	const unsigned plane = (unsigned)H * (unsigned)W;
	float acc[GSR_BG_LC][12];
#pragma unroll
	for (int j = 0; j < GSR_BG_LC; j++) {
#pragma unroll
		for (int i = 0; i < 12; i++) acc[j][i] = 0.f;
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (int y = y_lo + wave; y <= y_hi; y += GSR_BG_GATHER_WAVES) {
		float ty;
		const int cy = gsr_bg_cell(y, a.sy, GH, ty);
		const float wy = gsr_bg_hat(ny, cy, ty);
		if (wy == 0.f) continue;
		for (int x = x_lo + lane; x <= x_hi; x += 64) {
			float tx, tz;
			const int cx = gsr_bg_cell(x, a.sx, GW, tx);
			const float wxy = wy * gsr_bg_hat(nx, cx, tx);
			const unsigned o = (unsigned)y * (unsigned)W + (unsigned)x;
			const float v[4] = {a.img[o], a.img[plane + o], a.img[2 * plane + o], 1.f};
			const float G[3] = {a.G[o], a.G[plane + o], a.G[2 * plane + o]};
			bool inside;
			const int z = gsr_bg_level(v[0], v[1], v[2], a.lm, L, tz, inside);
			float P[12];
#pragma unroll
			for (int c = 0; c < 3; c++) {
				const float g = wxy * G[c];
#pragma unroll
				for (int k = 0; k < 4; k++) P[4 * c + k] = k < 3 ? g * v[k] : g;
			}
#pragma unroll
			for (int j = 0; j < GSR_BG_LC; j++) {
				const float wz = gsr_bg_hat(l0 + j, z, tz);
#pragma unroll
				for (int i = 0; i < 12; i++) acc[j][i] = __builtin_fmaf(wz, P[i], acc[j][i]);
			}
		}
	}
	// lanes, then waves in wave order
#pragma unroll
	for (int j = 0; j < GSR_BG_LC; j++) {
#pragma unroll
		for (int i = 0; i < 12; i++) {
			float s = acc[j][i];
#pragma unroll
			for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
			if (lane == 0) wsum[wave][j * 12 + i] = s;
		}
	}
	__syncthreads();
	if (threadIdx.x < 12 * GSR_BG_LC) {
		const int j = threadIdx.x / 12, ch = threadIdx.x % 12, l = l0 + j;
		float s = wsum[0][threadIdx.x];
#pragma unroll
		for (int q = 1; q < GSR_BG_GATHER_WAVES; q++) s += wsum[q][threadIdx.x];
		if (l < L) a.dst[(size_t)seg * a.ngrid + ((unsigned)((ch * L + l) * GH + ny) * (unsigned)GW + (unsigned)nx)] = s;
	}
}

// dL_dgrid = the segments' rows added in segment order, in double
__global__ void __launch_bounds__(256) gsr_bilagrid_segment_fold_kernel(unsigned n, int S, const float* __restrict__ rows, float* __restrict__ out)
{
	const unsigned e = blockIdx.x * 256u + threadIdx.x;
	if (e >= n) return;
	double t = 0.0;
	for (int s = 0; s < S; s++) t += rows[(size_t)s * n + e];
	out[e] = (float)t;
}

// tv: value partials {luma axis, y, x} per workgroup and the gradient, in one pass.  cz, cy, cx = 2 / (N count_a).
__global__ void __launch_bounds__(256) gsr_bilagrid_tv_kernel(unsigned n, int L, int GH, int GW, float cz, float cy, float cx,
                                                               const float* __restrict__ g, float* __restrict__ dg, float4* __restrict__ partial)
{
	__shared__ float wsum[4][3];
	const unsigned sy_ = (unsigned)GW, sz_ = (unsigned)GH * (unsigned)GW;
	float qz = 0.f, qy = 0.f, qx = 0.f;
#pragma unroll
	for (int j = 0; j < GSR_BG_TV_PER_THREAD; j++) {
		const unsigned i = (blockIdx.x * GSR_BG_TV_PER_THREAD + j) * 256u + threadIdx.x;
		if (i >= n) continue;
		const unsigned x = i % sy_, r = i / sy_, y = r % (unsigned)GH, z = (r / (unsigned)GH) % (unsigned)L;
		const float v = g[i];
		float grad = 0.f;
		if (x + 1 < (unsigned)GW) { const float d = g[i + 1] - v; qx = __builtin_fmaf(d, d, qx); grad -= cx * d; }
		if (x > 0) grad += cx * (v - g[i - 1]);
		if (y + 1 < (unsigned)GH) { const float d = g[i + sy_] - v; qy = __builtin_fmaf(d, d, qy); grad -= cy * d; }
		if (y > 0) grad += cy * (v - g[i - sy_]);
		if (z + 1 < (unsigned)L) { const float d = g[i + sz_] - v; qz = __builtin_fmaf(d, d, qz); grad -= cz * d; }
		if (z > 0) grad += cz * (v - g[i - sz_]);
		if (dg) dg[i] = grad;
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		qz += __shfl_down(qz, off, 64);
		qy += __shfl_down(qy, off, 64);
		qx += __shfl_down(qx, off, 64);
	}
	if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6][0] = qz; wsum[threadIdx.x >> 6][1] = qy; wsum[threadIdx.x >> 6][2] = qx; }
	__syncthreads();
	if (threadIdx.x == 0) {
		float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
		for (int q = 0; q < 4; q++) { t.x += wsum[q][0]; t.y += wsum[q][1]; t.z += wsum[q][2]; }
		partial[blockIdx.x] = t;
	}
}

// one workgroup folds the partials in a fixed order in double (gsr_loss_ext_finalize_kernel's order: strided per thread, lanes, waves)
__global__ void __launch_bounds__(256) gsr_bilagrid_tv_finalize_kernel(const float4* __restrict__ partial, int n, double iz, double iy, double ix,
                                                                        float* __restrict__ val)
{
	__shared__ double sw[4][3];
	double v[3] = {0.0, 0.0, 0.0};
	for (int i = threadIdx.x; i < n; i += 256) { const float4 p = partial[i]; v[0] += p.x; v[1] += p.y; v[2] += p.z; }
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
		for (int q = 0; q < 3; q++) v[q] += __shfl_down(v[q], off, 64);
	}
	if ((threadIdx.x & 63) == 0) {
#pragma unroll
		for (int q = 0; q < 3; q++) sw[threadIdx.x >> 6][q] = v[q];
	}
	__syncthreads();
	if (threadIdx.x == 0)
		val[0] = (float)((sw[0][0] + sw[1][0] + sw[2][0] + sw[3][0]) * iz + (sw[0][1] + sw[1][1] + sw[2][1] + sw[3][1]) * iy +
		                 (sw[0][2] + sw[1][2] + sw[2][2] + sw[3][2]) * ix);
}

// ---- host side ----
long long gsr_bilagrid_tiles(int H, int W)
{
	return (long long)((W + GSR_BG_TX - 1) / GSR_BG_TX) * ((H + GSR_BG_TY - 1) / GSR_BG_TY);
}

static long long gsr_bg_units(int L, int GH, int GW) { return (long long)GH * GW * ((L + GSR_BG_LC - 1) / GSR_BG_LC); }

int gsr_bilagrid_segments(int H, int L, int GH, int GW)
{
	const long long m = gsr_bg_units(L, GH, GW);
	long long S = (GSR_BG_FILL + m - 1) / m;
	if (S > GSR_BG_MAX_SEGMENTS) S = GSR_BG_MAX_SEGMENTS;
	if (S > H) S = H;
	return (int)S;
}

long long gsr_bilagrid_gather_blocks(int H, int L, int GH, int GW) { return gsr_bg_units(L, GH, GW) * gsr_bilagrid_segments(H, L, GH, GW); }

// Room for the segments' rows: S rows of 12 L GH GW floats with S <= ceil(FILL / m), m = GH GW ceil(L / LC) and 12 L <= 12 LC ceil(L / LC),
// is less than (FILL + m) 12 LC floats -- a bound that grows with every argument, which S times the grid does not (S falls as m grows).
size_t gsr_bilagrid_scratch_size(int H, int W, int L, int GH, int GW)
{
	(void)H; (void)W;
	return gsr_align_up((size_t)(GSR_BG_FILL + gsr_bg_units(L, GH, GW)) * 12 * GSR_BG_LC * sizeof(float));
}

static GsrBgSlice gsr_bg_slice_args(const gsr_bilagrid_args& a, const float* G, float* dst, size_t* lds_bytes)
{
	GsrBgSlice k;
	k.H = a.H; k.W = a.W; k.L = a.L; k.GH = a.GH; k.GW = a.GW;
	k.tiles_x = (a.W + GSR_BG_TX - 1) / GSR_BG_TX;
	k.sx = (float)a.W; k.sy = (float)a.H; k.lm = (float)(a.L - 1);
	// the most nodes a tile's pixels can touch along an axis: the span of its pixel centres in cells, the far corner, and one each for
	// the floor at either end and for rounding
	const long long bx = std::min<long long>(a.GW, (long long)((GSR_BG_TX - 1) * (double)(a.GW - 1) / a.W) + 4);
	const long long by = std::min<long long>(a.GH, (long long)((GSR_BG_TY - 1) * (double)(a.GH - 1) / a.H) + 4);
	const long long row = bx * a.L * 12 * (long long)sizeof(float);
	*lds_bytes = 2 * row > GSR_BG_LDS_BYTES ? 0 : (size_t)std::min<long long>(by * row, GSR_BG_LDS_BYTES);
	k.lds_floats = (int)(*lds_bytes / sizeof(float));
	k.grid = a.grid; k.img = a.img; k.G = G; k.dst = dst;
	return k;
}

void gsr_launch_bilagrid_slice(const gsr_bilagrid_args& a, hipStream_t s)
{
	GsrProfScope p(s, "bilagrid_slice");
	size_t lds;
	const GsrBgSlice k = gsr_bg_slice_args(a, nullptr, a.out, &lds);
	hipLaunchKernelGGL(gsr_bilagrid_pixel_kernel<false>, dim3((unsigned)gsr_bilagrid_tiles(a.H, a.W)), dim3(GSR_BG_THREADS), lds, s, k);
}

void gsr_launch_bilagrid_backward(const gsr_bilagrid_args& a, hipStream_t s)
{
	GsrProfScope p(s, "bilagrid_backward");
	if (a.dL_dimg) {
		size_t lds;
		const GsrBgSlice k = gsr_bg_slice_args(a, a.dL_dout, a.dL_dimg, &lds);
		hipLaunchKernelGGL(gsr_bilagrid_pixel_kernel<true>, dim3((unsigned)gsr_bilagrid_tiles(a.H, a.W)), dim3(GSR_BG_THREADS), lds, s, k);
	}
	if (a.dL_dgrid) {
		const int S = gsr_bilagrid_segments(a.H, a.L, a.GH, a.GW);
		GsrBgGather k;
		k.H = a.H; k.W = a.W; k.L = a.L; k.GH = a.GH; k.GW = a.GW;
		k.nch = (a.L + GSR_BG_LC - 1) / GSR_BG_LC;
		k.RS = (a.H + S - 1) / S;
		k.sx = (float)a.W; k.sy = (float)a.H; k.lm = (float)(a.L - 1);
		k.img = a.img; k.G = a.dL_dout;
		k.dst = S > 1 ? (float*)a.scratch : a.dL_dgrid;
		k.ngrid = 12u * (unsigned)a.L * (unsigned)a.GH * (unsigned)a.GW;
		hipLaunchKernelGGL(gsr_bilagrid_grid_backward_kernel, dim3((unsigned)gsr_bg_units(a.L, a.GH, a.GW), S), dim3(GSR_BG_GATHER_THREADS), 0, s, k);
		if (S > 1)
			hipLaunchKernelGGL(gsr_bilagrid_segment_fold_kernel, dim3((k.ngrid + 255u) / 256u), dim3(256), 0, s, k.ngrid, S, (const float*)a.scratch,
			                   a.dL_dgrid);
	}
}

static unsigned gsr_bg_tv_blocks(long long n) { return (unsigned)((n + 256 * GSR_BG_TV_PER_THREAD - 1) / (256 * GSR_BG_TV_PER_THREAD)); }

size_t gsr_bilagrid_tv_scratch_size(int N, int L, int GH, int GW)
{
	return gsr_align_up((size_t)gsr_bg_tv_blocks((long long)N * 12 * L * GH * GW) * sizeof(float4));
}

void gsr_launch_bilagrid_tv(int N, int L, int GH, int GW, const float* grids, float* val, float* dL_dgrids, void* scratch, hipStream_t s)
{
	GsrProfScope p(s, "bilagrid_tv");
	const long long n = (long long)N * 12 * L * GH * GW;
	const unsigned blocks = gsr_bg_tv_blocks(n);
	// count_a: the differences along axis a in one image's grid
	const double nz = 12.0 * (L - 1) * GH * GW, ny = 12.0 * L * (GH - 1) * GW, nx = 12.0 * L * GH * (GW - 1);
	const double iz = 1.0 / (N * nz), iy = 1.0 / (N * ny), ix = 1.0 / (N * nx);
	hipLaunchKernelGGL(gsr_bilagrid_tv_kernel, dim3(blocks), dim3(256), 0, s, (unsigned)n, L, GH, GW, (float)(2.0 * iz), (float)(2.0 * iy),
	                   (float)(2.0 * ix), grids, dL_dgrids, (float4*)scratch);
	hipLaunchKernelGGL(gsr_bilagrid_tv_finalize_kernel, dim3(1), dim3(256), 0, s, (const float4*)scratch, (int)blocks, iz, iy, ix, val);
}
