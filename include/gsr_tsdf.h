/*
 * gsr_tsdf.h -- TSDF fusion of rendered depth maps and the extraction of a triangle mesh from the fused field: the last step of the
 * geometry-regularised methods (2DGS, PGSR, RaDe-GS, Gaussian surfels), which they take from Open3D's TSDF volumes and marching cubes.
 * Entry points beside the core ABI of gsr.h, whose declarations they leave as they are.  Choosing the bounds and the resolution of the
 * volume, and what becomes of the mesh afterwards (its largest components, a decimation), stays with the caller.
 *
 * The volume (gsr_tsdf_grid): nx x ny x nz sample points ("nodes") at origin + (i, j, k) voxel_size, node index n = i + nx (j + ny k),
 * x fastest, nx ny nz < 2^31.  It is held as planes of float32 on the device, each of nx ny nz elements:
 *   wsum = sum w        dsum = sum w tsdf        csum [3][nodes] = sum w rgb, optional
 * Sums, not running means: the value dsum / wsum is formed once, at extraction.  Dense only.
 *
 * gsr_tsdf_integrate -- one launch for the whole batch of C cameras: one thread per node keeps the node's sums in registers and walks
 * the camera records (the packed 80-byte gsr_filter3d_camera of gsr_filter3d.h) through wave-uniform loads; every plane is read once
 * and, where a camera touched the node, written once.  depth [C][H][W], color [C][3][H][W] or NULL, weight [C][H][W] or NULL, float32 on
 * the device.  For node (i, j, k) and camera c, in float32 and in exactly these operations (the unit is compiled without contraction):
 *   x = fma(i, voxel_size, origin_x), y and z alike
 *   p_j = fma(R_j0, x, fma(R_j1, y, fma(R_j2, z, t_j)))                      skip unless p_z > 0
 *   r = rcp(p_z) (the device's reciprocal, within 1 ulp);  U = fma(p_x r, fx, cx),  V = fma(p_y r, fy, cy)
 *       in the convention of gsr_camera_model.h: the origin at the corner of the first pixel, pixel i covers [i, i + 1)
 *   pixel = (floor(U), floor(V))                                             skip unless 0 <= U < W and 0 <= V < H
 *   d = depth[c][pixel]: the nearest pixel, no interpolation across depth edges
 *                                                                            skip unless d is finite, d > 0 and d <= depth_trunc
 *   sdf = d - p_z, the projective distance along z that the library's depth maps measure
 *                                                                            skip if sdf < -sdf_trunc
 *   tsdf = min(1, sdf * inv), inv = fp32(1 / sdf_trunc) formed on the host in double
 *   w = weight[c][pixel], or 1                                               skip unless w is finite and w > 0
 *   wsum = wsum + w;  dsum = fma(w, tsdf, dsum);  csum_k = fma(w, color[c][k][pixel], csum_k)
 * The additions start from the planes' current values and run in ascending camera order: a call with cameras 0..4 leaves the bits of a
 * call with 0..1 followed by a call with 2..4.  A node no camera touches keeps its bits.  W and H are those of the tensors (the bounds
 * of every pixel access); where `cameras_host`, the same records in host memory, is given, each record's W and H must equal them.
 *
 * gsr_tsdf_mesh_plan / gsr_tsdf_mesh_emit -- marching tetrahedra, two calls because the counts must reach the host before the outputs
 * can be allocated.  A node is valid where wsum >= min_weight; its value is dsum / wsum, formed in double; it is inside where the value
 * is < 0 (exactly 0 is outside).  Every cell is split into the six tetrahedra around its diagonal (0,0,0)-(1,1,1) (Freudenthal / Kuhn):
 * tetrahedron T of cell (i, j, k), T = 0..5 for the axis orders xyz, xzy, yxz, yzx, zxy, zyx, has the corners o, o + e_a, o + e_a + e_b,
 * o + (1,1,1) for the axis order (a, b, c): its "path".  The split is the same in every cell, so neighbouring cells agree on the
 * diagonals of their common face.  A tetrahedron emits triangles only where all four corners are valid: none where all are on one
 * side, one where one corner is apart from the other three, two where two are inside.
 *   Vertices: one per crossed grid edge (both ends valid, one inside and one not), owned by the edge's lower node; a node owns seven
 *     kinds of edge, in this order: +x, +y, +z, +xy, +yz, +xz, +xyz.  Position: with v0 the value at the lower and v1 at the upper node,
 *     t = v0 / (v0 - v1), always from the lower to the upper node; coordinate = origin + (index + t) voxel_size along the axes the edge
 *     moves in, origin + index voxel_size along the others; colour = c0 + t (c1 - c0) with c = csum / wsum.  All in double from the
 *     float32 inputs, rounded once.  A crossed edge next to an invalid node may belong to no emitting tetrahedron: its vertex is
 *     written and no face names it.
 *   Faces: counter-clockwise seen from the positive side (free space, where the cameras were): the normal points out of the surface.
 *     Two corners a < b inside and c < d outside, numbered along the path: the quadrilateral of the vertices on the edges ac, ad, bd, bc
 *     (in this cyclic order) is split along the diagonal ac-bd; the first triangle holds ad, the second bc, both begin at ac.
 *   Order: vertices ascend in (node index, edge kind), faces in (cell index, tetrahedron, triangle); a cell's index is that of its
 *     node (i, j, k).  No atomics: the mesh is bit-identical from run to run.
 *   plan: a workgroup of GSR_TSDF_THREADS threads counts the crossed edges and the triangles of as many nodes and stores each node's
 *     7-bit crossing mask; one workgroup scans the workgroup totals in index order; the two totals (V, F) are copied to the host and the
 *     stream is synchronised: the read-back is part of the call.  `plan` (host memory) is filled in for emit.
 *   emit: with the plan and V, F as the caller allocated for: (1) every node's first vertex id and the vertices; (2) the faces, whose
 *     vertex ids are the owner node's first id plus the rank of the edge's kind in the owner's mask.  The planes must not have changed
 *     since the plan.  V = 0 launches nothing.  No access leaves a tensor whatever the counts are.
 *   scratch: gsr_tsdf_mesh_scratch_bytes(nodes) bytes, at most 8 per node (5 per node, 8 per workgroup, 16); contents irrelevant before
 *     plan, needed unchanged by emit.
 *   Outputs: vertices [V][3] float32, colors [V][3] float32 or NULL, faces [F][3] int32.
 *
 * Refused with GSR_ERR_INVALID_ARGUMENT before any device work, with a message that starts with the function's name: a NULL required
 * pointer; a dimension below 1 (integrate) or below 2 (plan); nx ny nz beyond 2^31 - 1; an origin that is not finite; voxel_size,
 * sdf_trunc or min_weight not finite and positive; depth_trunc NaN or not positive (+inf is allowed); C < 1; H or W below 1 or
 * beyond 2^24 (pixel coordinates are compared in float32) or H W beyond 2^31 - 1; color without csum; a record of cameras_host whose
 * W or H differ from the tensors'; V or F beyond 2^31 - 1 or negative; V or F that differ from the plan's; colors without csum; a
 * scratch pointer that is not 8-byte aligned; a plan that was not filled in by gsr_tsdf_mesh_plan.
 * Profiling stages (gsr_profile_*): "tsdf_integrate", "tsdf_mesh_plan", "tsdf_mesh_emit".
 */
#ifndef GSR_TSDF_H_INCLUDED
#define GSR_TSDF_H_INCLUDED
#include "gsr.h"
#include "gsr_filter3d.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_TSDF_THREADS 256                /* workgroup size of every kernel but the scan; the nodes of one workgroup */
#define GSR_TSDF_BRICK_X 8                  /* integrate: a workgroup takes 8 x 8 x 4 nodes, a wave 8 x 8 x 1 */
#define GSR_TSDF_BRICK_Y 8
#define GSR_TSDF_BRICK_Z 4
#define GSR_TSDF_PLAN_MAGIC 0x74736466      /* gsr_tsdf_mesh_plan_t.magic once gsr_tsdf_mesh_plan has filled it in */

typedef struct gsr_tsdf_grid {
    int nx, ny, nz;
    float origin[3];
    float voxel_size;
} gsr_tsdf_grid;

typedef struct gsr_tsdf_mesh_plan_t {       /* host memory; written by gsr_tsdf_mesh_plan, read by gsr_tsdf_mesh_emit */
    long long V, F;                         /* vertices and faces of the mesh */
    gsr_tsdf_grid grid;
    const float *wsum, *dsum;
    void* scratch;
    float min_weight;
    int magic;
} gsr_tsdf_mesh_plan_t;

int gsr_tsdf_integrate(const gsr_tsdf_grid* grid, float* wsum, float* dsum, float* csum /* or NULL */, int C,
                       const gsr_filter3d_camera* cameras /* [C] on the device */, const gsr_filter3d_camera* cameras_host /* [C] or NULL */,
                       int H, int W, const float* depth, const float* color /* or NULL */, const float* weight /* or NULL */,
                       float sdf_trunc, float depth_trunc, void* stream);
size_t gsr_tsdf_mesh_scratch_bytes(long long nodes);   /* 0 for a size that is not valid */
int gsr_tsdf_mesh_plan(const gsr_tsdf_grid* grid, const float* wsum, const float* dsum, float min_weight, void* scratch,
                       gsr_tsdf_mesh_plan_t* plan, void* stream);
int gsr_tsdf_mesh_emit(const gsr_tsdf_mesh_plan_t* plan, long long V, long long F, const float* csum /* or NULL */, float* vertices,
                       float* colors /* or NULL */, int32_t* faces, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* GSR_TSDF_H_INCLUDED */
