/*
 * gsr_knn.h -- the neighbour graph of a point cloud: an exact K-nearest-neighbour search, the reverse adjacency of its index table
 * and a neighbour gather whose backward is a fixed-order sum.  Entry points beside the core ABI of gsr.h, whose declarations they
 * leave as they are (gsr_knn_mean_dist2, the scale initialiser, stays what it is).  What SuGaR, Dynamic 3D Gaussians, the isometry
 * and rigidity regularisers and outlier pruning need and simple-knn does not return: indices, any K up to 32, a second point set.
 *
 * All arrays are on the device: float32 and int32, row-major, contiguous.
 *
 * gsr_knn_search -- for every query the K nearest reference points, 1 <= K <= GSR_KNN_MAX_K.
 *   points [P][3]; queries [Q][3], or NULL = the self-set form: the queries are the points (Q must equal P) and a point is left out
 *   of its own list by position, not by value, so coincident points count with distance 0.  In the two-set form nothing is left out.
 *   dist2 [Q][K] ascending, idx [Q][K] indices into `points` as the caller holds them.
 *   distance: dx = c.x - q.x, dy, dz likewise, then dx*dx + dy*dy + dz*dz left to right in float32, no contraction -- as
 *   gsr_knn_mean_dist2 forms it, so ((d0 + d1) + d2) / 3 of K = 3 has that call's bits.
 *   order: lexicographic in (distance, index): among equal distances the smaller index comes first, inside the K as well as at the
 *   K-th place.  The result is unique.  Places that have no neighbour (fewer than K candidates) hold +inf and -1.
 *   Non-finite coordinates give unspecified values; the search still ends and touches nothing outside its arrays.
 *   scratch: gsr_knn_search_scratch_bytes(P, Q) bytes, Q = the rows of `queries` (0 for the self-set form); 16-byte aligned, contents
 *   irrelevant, free for reuse once the call's work on the stream has finished.  Bitwise reproducible.
 *
 * gsr_knn_graph_build -- the edges of an index table grouped by target.  idx [E] with values in [-1, P), E = Q*K; edge e = q*K + k
 *   points at idx[e], -1 = no edge (a value outside [-1, P) is treated as -1).  offsets [P + 1]; edges has room for E ids, of which
 *   the first offsets[P] are written: the ids with a target, grouped by target j at edges[offsets[j] .. offsets[j + 1]) and
 *   ascending inside a target -- a stable sort of the edge ids by target.  num_valid, when not NULL, receives offsets[P] on the
 *   device.  Integer work only.  scratch: gsr_knn_graph_scratch_bytes(E, P).
 *
 * gsr_knn_gather -- out[q][k][c] = x[idx[q][k]][c] for x [P][C], any C >= 1; zeros where idx is -1.  idx must lie in [-1, P).
 *
 * gsr_knn_gather_backward -- grad_x[j][c] = the float32 sum, started at 0, of grad_out[e][c] over edges[offsets[j] ..
 *   offsets[j + 1]) in that order (ascending edge id).  One thread owns each (j, c) and adds sequentially: no atomics, bitwise
 *   reproducible, and equal bit for bit to the sequential sum in that order.  A row with no edge gets 0.
 *
 * Refused with GSR_ERR_INVALID_ARGUMENT (-1) before any device work, with a gsr_last_error() text that starts with the function's
 * name: a negative count; K outside 1 .. GSR_KNN_MAX_K; Q != P in the self-set form; a NULL pointer where the count it belongs to is
 * not zero; scratch that is not 16-byte aligned; Q*K or a product with C beyond what the 32-bit grids index (E < 2^31,
 * E*C and P*C < 2^39).  A call with nothing to do (P == 0 or Q == 0 in the search, E == 0 or C == 0 in the gather, P == 0 or C == 0
 * in its backward) returns 0 whatever the pointers; gsr_knn_graph_build with E == 0 or P == 0 writes zeros to offsets [P + 1]
 * where it is not NULL.
 * Profiling stages (gsr_profile_*): "knn_search", "knn_graph_build", "knn_gather", "knn_gather_bwd".
 */
#ifndef GSR_KNN_H_INCLUDED
#define GSR_KNN_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_KNN_MAX_K 32

size_t gsr_knn_search_scratch_bytes(int P, int Q);   /* 0 for P <= 0 */
int gsr_knn_search(int P, const float* points, int Q, const float* queries /* or NULL */, int K, float* dist2, int* idx, void* scratch,
                   void* stream);
size_t gsr_knn_graph_scratch_bytes(int E, int P);    /* 0 for E <= 0 or P <= 0 */
int gsr_knn_graph_build(int E, const int* idx, int P, int* offsets, int* edges, int* num_valid /* or NULL */, void* scratch, void* stream);
int gsr_knn_gather(int Q, int K, int C, const float* x, const int* idx, float* out, void* stream);
int gsr_knn_gather_backward(int P, int C, const int* offsets, const int* edges, const float* grad_out, float* grad_x, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* GSR_KNN_H_INCLUDED */
