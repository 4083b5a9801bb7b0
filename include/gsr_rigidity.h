/*
 * gsr_rigidity.h -- the neighbour-rigidity losses of Dynamic 3D Gaussians (Luiten et al., 3DV 2024: rigid, rotation, isometry) over
 * the neighbour graph of gsr_knn.h: the three terms, their weighted total and its gradients with respect to the positions and the
 * raw rotations, in one pass over the edges and one fixed-order sum per point.  An entry point beside the core ABI of gsr.h.
 *
 * All arrays are on the device: float32 and int32, row-major, contiguous; 4-byte alignment is enough for all but scratch.
 * Quaternions are (w, x, y, z).
 *
 *   xyz [P][3], rotation [P][4]    the current leaves; the rotation is raw (not normalised)
 *   idx [P][K]                     the neighbour table, values in [-1, P), -1 = no edge (a value outside counts as -1)
 *   prev_offset [P][K][3]          o_ik = x_j - x_i at capture time
 *   prev_dist [P][K]               d_ik = |o_ik|
 *   weight [P][K]                  w_ik
 *   prev_inv_rot [P][4]            p_i: the conjugate of the normalised rotation at capture time
 *   offsets [P + 1], edges         the reverse adjacency of idx as gsr_knn_graph_build writes it; offsets[P] = N_e, the number of
 *                                  valid edges.  edges is read only when a gradient is asked for.
 * The tables are read in this (P, K, .) layout, the layout of the paper's own arrays: a point is worked on by a group of lanes that
 * reads consecutive places of its rows, so no packed form is needed.  Places where idx is -1 are never read in prev_offset,
 * prev_dist and weight.
 *
 * For a valid edge (i, k), j = idx[i][k]:  q_i = r_i / |r_i|, rel_i = q_i (x) p_i (Hamilton product), R_i = the rotation matrix of
 * rel_i / |rel_i|, c = x_j - x_i,
 *   rigid_ik = sqrt(w |R_i^T c - o|^2 + 1e-20),  rot_ik = sqrt(w |rel_j - rel_i|^2 + 1e-20),
 *   iso_ik = sqrt(w (sqrt(|c|^2 + 1e-20) - d)^2 + 1e-20).
 * Each term is the sum over the valid edges divided by N_e (with no -1 in the table: the mean over P K); N_e = 0 gives 0 and zero
 * gradients.  values [4] = {total, rigid, rot, iso}, total = w_rigid rigid + w_rot rot + w_iso iso.
 * grad_xyz [P][3] and grad_rot [P][4], each may be NULL: the gradients of the total, through the normalisation of r, the product with
 * p and the normalisation inside the rotation matrix; row i as the centre of its K edges and as the neighbour of every edge that
 * points at it.  With both NULL no per-edge row is stored and the per-point sum is not launched.  A zero quaternion gives unspecified
 * values; nothing outside the arrays is touched.
 * Order of every sum: a point's own edges per lane in ascending k and the lanes by a fixed tree; the incoming edges of row j over
 * edges[offsets[j] .. offsets[j + 1]) in ascending edge id, then the centre part; the values per workgroup, then in double in a fixed
 * order.  No atomics: bitwise reproducible.
 * scratch: gsr_rigidity_scratch_bytes(P, K) bytes (28 bytes per edge, 44 per point and 12 per workgroup), 16-byte aligned, contents
 * irrelevant, free for reuse once the call's work on the stream has finished.
 *
 * Refused with GSR_ERR_INVALID_ARGUMENT (-1) before any device work, with a gsr_last_error() text that starts with the function's
 * name: a negative count; K above GSR_RIGIDITY_MAX_K; values NULL; P*K >= 2^31; with P > 0 and K > 0, a NULL array (edges only when
 * a gradient is asked for) or scratch that is NULL or not 16-byte aligned.  P == 0 or K == 0 writes zeros to values (and to the
 * gradients that are given) and returns 0 whatever the other pointers.  gsr_rigidity_scratch_bytes is 0 for such counts and for
 * counts the call refuses.
 * Profiling stages (gsr_profile_*): "rigidity_edges", "rigidity_fold".
 */
#ifndef GSR_RIGIDITY_H_INCLUDED
#define GSR_RIGIDITY_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_RIGIDITY_MAX_K 32

size_t gsr_rigidity_scratch_bytes(int P, int K);
int gsr_rigidity_loss(int P, int K, const float* xyz, const float* rotation, const int* idx, const float* prev_offset, const float* prev_dist,
                      const float* weight, const float* prev_inv_rot, const int* offsets, const int* edges /* or NULL without gradients */,
                      float w_rigid, float w_rot, float w_iso, float* values, float* grad_xyz /* or NULL */, float* grad_rot /* or NULL */,
                      void* scratch, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* GSR_RIGIDITY_H_INCLUDED */
