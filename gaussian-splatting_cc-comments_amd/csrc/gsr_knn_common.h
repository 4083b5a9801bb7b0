// gsr_knn_common.h -- what knn.hip (distCUDA2) and knn_graph.hip (the K-NN search) share: the box records, the device helpers of the
// pruning tests and the host-side steps that put a cloud into Morton order.  The kernels of those steps live in knn.hip.
#ifndef GSR_KNN_COMMON_H_INCLUDED
#define GSR_KNN_COMMON_H_INCLUDED
#include <float.h>

#include "gsr_internal.h"

#define GSR_KNN_BOX 256
#define GSR_KNN_SUPER 16  // boxes per super box

struct GsrKnnBox { float mnx, mny, mnz, mxx, mxy, mxz; };

__device__ __forceinline__ float gsr_wave_min(float v)
{
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
	return v;
}
__device__ __forceinline__ float gsr_wave_max(float v)
{
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
	return v;
}

// squared distance from p to the box (0 inside), simple_knn.cu:116-126
__device__ __forceinline__ float gsr_point_box_dist2(const GsrKnnBox& b, float x, float y, float z)
{
	float dx = 0.f, dy = 0.f, dz = 0.f;
	if (x < b.mnx || x > b.mxx) dx = fminf(fabsf(x - b.mnx), fabsf(x - b.mxx));
	if (y < b.mny || y > b.mxy) dy = fminf(fabsf(y - b.mny), fabsf(y - b.mxy));
	if (z < b.mnz || z > b.mxz) dz = fminf(fabsf(z - b.mnz), fabsf(z - b.mxz));
	return dx * dx + dy * dy + dz * dz;
}
// lower bound of the squared distance between any point of q and any point of b; never above the fp32
// point-box distance of a point inside q (same expression shape, monotone rounding)
__device__ __forceinline__ float gsr_box_box_dist2(const GsrKnnBox& b, const GsrKnnBox& q)
{
	const float dx = fmaxf(0.f, fmaxf(b.mnx - q.mxx, q.mnx - b.mxx));
	const float dy = fmaxf(0.f, fmaxf(b.mny - q.mxy, q.mny - b.mxy));
	const float dz = fmaxf(0.f, fmaxf(b.mnz - q.mxz, q.mnz - b.mxz));
	return dx * dx + dy * dy + dz * dz;
}

// ---- host side (knn.hip) ------------------------------------------------------------------------------------
struct GsrKnnScratch {
	GsrKnnBox* bounds;
	GsrKnnBox* partial;
	uint32_t *codes, *codes_alt, *idx, *idx_alt;
	float4* sorted;
	GsrKnnBox* boxes;
	GsrKnnBox* supers;
	void* table;
	size_t total;
};
GsrKnnScratch gsr_knn_carve(void* base, int P);
// bounds of the cloud -> k.bounds
void gsr_knn_cloud_bounds(int P, const float* points, const GsrKnnScratch& k, hipStream_t s);
// the n points in the Morton order of their cells inside *bounds -> k.sorted {x, y, z, original index}, k.boxes, k.supers;
// returns the sorted codes (k.codes or k.codes_alt)
const uint32_t* gsr_knn_morton_order(int n, const float* pts, const GsrKnnBox* bounds, const GsrKnnScratch& k, hipStream_t s);
#endif
