/*
 * gsr_vq.h -- vector quantisation of the rows of a matrix: a nearest-code search whose scores run on the fp32-input matrix cores
 * and a fixed-order centroid update, the two steps of Lloyd's k-means and of every codebook compression of a Gaussian model
 * (features_rest D = 45, scales + rotations D = 7, DC colour D = 3).  Entry points beside the core ABI of gsr.h, whose declarations
 * they leave as they are.  Nothing of size N x K is ever stored.
 *
 * All arrays are on the device: float32 and int32, row-major, contiguous.
 *
 * gsr_vq_assign -- for every row of x [N][D] the nearest row of codebook [K][D]; 1 <= D <= GSR_VQ_MAX_D, 1 <= K <= GSR_VQ_MAX_K.
 *   The score s_ij of row i against code j, in float32, operation by operation:
 *     c2_j = the chain acc = fmaf(c_jk, c_jk, acc) for k = 0 .. D-1 ascending, started at +0;
 *     s_ij = the chain acc = fmaf(-2 * x_ik, c_jk, acc) for k = 0 .. D-1 ascending, started at c2_j (-2 * x is an exact scaling).
 *   s_ij = |c_j|^2 - 2 x_i . c_j orders the codes of one row as the squared distance does (|x_i|^2 is common to them).  The chain is
 *   what v_mfma_f32_32x32x2_f32 computes with c2_j as its C input; D is padded with zeros to the instruction's k step, and
 *   fmaf(0, 0, acc) = acc leaves the bits alone.
 *   idx [N]: the j that minimises (s_ij, j) lexicographically, the scores compared as floats (-0 equals +0): among equal scores the
 *   smallest index wins.  The running best starts at (+inf, -1) and is replaced only on `<`, so a row whose every score is NaN or
 *   +inf gets -1.
 *   dist2 [N], or NULL: the chain acc = fma(d, d, acc) in double with d = double(x_ik) - double(c_jk), k ascending from +0, for the
 *   chosen code, rounded once to float32; NaN where idx is -1.  It does not come from the expanded form and carries no cancellation.
 *   scratch: gsr_vq_assign_scratch_bytes(N, D, K) bytes, 16-byte aligned, contents irrelevant, free for reuse once the call's work on
 *   the stream has finished.  Bitwise reproducible.
 *
 * gsr_vq_update -- every code moves to the weighted mean of its members.  offsets [K + 1], members [offsets[K]]: the output of
 *   gsr_knn_graph_build over idx (E = N, P = K), i.e. the rows of code j at members[offsets[j] .. offsets[j + 1]) in ascending row
 *   order, rows of idx = -1 left out.  weight [N] >= 0, or NULL = 1.  For code j and column d, in double:
 *     S_d = S_d + double(w_i) * double(x_id) and W = W + double(w_i), the members one after the other in list order, from +0
 *     (every product is exact in double); then codebook[j][d] = float32(S_d / W).
 *   Long lists are split in a way that depends on the list's length L alone: P = min(16, max(1, L / 256)) parts (integer division)
 *   of Q = ceil(L / P) consecutive members, the last one shorter; each part is added as above from +0 and the parts' sums are then
 *   added in ascending part order, ((part_0 + part_1) + part_2) ..., in double.  Below 512 members P is 1: the plain sequential sum.
 *   A code with no member, or with W == 0, keeps its bits.  count [K] (int32, or NULL) receives the number of members, wsum [K]
 *   (float32, or NULL) float32(W).  One lane owns each (code, column) and adds sequentially: no atomics, bitwise reproducible.
 *
 * Refused with GSR_ERR_INVALID_ARGUMENT (-1) before any device work, with a gsr_last_error() text that starts with the function's
 * name: a negative count; D outside 1 .. GSR_VQ_MAX_D; K outside 1 .. GSR_VQ_MAX_K; a NULL pointer where the count it belongs to is
 * not zero; scratch that is not 16-byte aligned.  A call with N == 0 returns 0 whatever the pointers (the update then leaves the
 * codebook alone and writes nothing).
 * Profiling stages (gsr_profile_*): "vq_assign", "vq_update".
 */
#ifndef GSR_VQ_H_INCLUDED
#define GSR_VQ_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_VQ_MAX_D 64
#define GSR_VQ_MAX_K 65536

size_t gsr_vq_assign_scratch_bytes(int N, int D, int K);   /* 0 for arguments outside the limits */
int gsr_vq_assign(int N, int D, const float* x, int K, const float* codebook, int* idx, float* dist2 /* or NULL */, void* scratch,
                  void* stream);
int gsr_vq_update(int N, int D, const float* x, const float* weight /* or NULL */, int K, const int* offsets, const int* members,
                  float* codebook, int* count /* or NULL */, float* wsum /* or NULL */, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* GSR_VQ_H_INCLUDED */
