/*
 * gsr_densify.h -- the structural edit of adaptive density control (the reference's GaussianModel.densify_and_prune,
 * scene/gaussian_model.py:394-594; gsplat's DefaultStrategy) as one compaction: given one action code per row, every tensor of the
 * optimiser is written once into new storage.  Entry points beside the core ABI of gsr.h, whose declarations they leave as they are.
 * The policy -- when to densify, which rows get which code -- stays with the caller.
 *
 * action [P] uint8 on the device, one code per row:
 *   GSR_DENSIFY_KEEP  0  the row survives with its moments
 *   GSR_DENSIFY_PRUNE 1  no output row
 *   GSR_DENSIFY_CLONE 2  the row survives with its moments, plus one copy
 *   GSR_DENSIFY_SPLIT 3  the row is replaced by GSR_DENSIFY_SPLIT_N = 2 children
 * A code above 3 is counted in totals[3] and otherwise treated as PRUNE.  With K the number of KEEP and CLONE rows, C of CLONE rows
 * and S of SPLIT rows the output has P' = K + C + 2 S rows, in the order the reference's clone, split, prune sequence ends with:
 *   [0, K)            survivors, in index order
 *   [K, K + C)        clone copies, in the index order of their sources
 *   [K + C, +S)       the first child of every split row, in source order
 *   [K + C + S, +S)   the second child of every split row, in source order
 *
 * Groups as gsr_mcmc_group, with an output beside every input: param [P][row] -> out_param [P'][row], exp_avg and exp_avg_sq given
 * together or both NULL, row >= 0 in 4-byte words.  A group with row = 0 is skipped.  Groups are copied as 32-bit words, so float32
 * statistics and int32 tables ride along as groups without moments.  Per output row d with source i:
 *   survivor (d < K)     param and both moments carry the bits of row i
 *   clone copy or child  param carries the bits of row i, or +0.0 where the group's zero_new is set; both moments are +0.0
 *   child k (0 or 1) of the j-th split row, n = noise[k S + j] (noise [2 S][3]: the caller's standard-normal draw):
 *     xyz_group:    xyz_i + R(q_i / |q_i|) (exp(ls_i) * n), R the matrix every other kernel of the library builds, the displacement
 *                   complete in fp32 before it meets the position
 *     scale_group:  fp32((double)ls_i - GSR_DENSIFY_LOG_SHRINK): one exactly rounded double subtraction and one rounding
 *   (zero_new set on the xyz or the scale group wins over the children's arithmetic.)
 *
 * Two calls, because P' must reach the host before the outputs can be allocated:
 *   gsr_densify_plan   a workgroup of 256 threads counts (K, C, S, bad) over GSR_DENSIFY_PLAN_ROWS rows; one workgroup then scans the
 *                      workgroup totals in index order (it loops where there are more totals than threads), leaves the exclusive
 *                      bases in `scratch` (gsr_densify_scratch_bytes(P) bytes) and totals = {K, C, S, bad} as int32 on the device.
 *   gsr_densify_apply  with K, C, S as read back: every workgroup re-scans its own rows from its base and writes src_of [P'] (int32
 *                      scratch), each source row its one or two entries; then one launch per group streams over the group's output
 *                      words, out[d row + c] = in[src_of[d] row + c].
 * No atomics, no workgroup waits for another inside a launch, every output is bit-identical from run to run.  The input tensors are
 * only read.  K, C and S that are not the plan's make no access outside the tensors: entries beyond P' are not written, and an output
 * row whose map entry names no input row is left unwritten.  P' = 0 is allowed and launches nothing in apply.
 *
 * Refused with GSR_ERR_INVALID_ARGUMENT before any device work, with a message that starts with the function's name: a NULL required
 * pointer; P < 1; negative K, C or S, C > K or K + S > P; ngroups outside 1 .. GSR_DENSIFY_MAX_GROUPS; a negative row; one moment
 * without the other; a group index that names no group (-1 is allowed while S = 0) or one group twice; an xyz or scale row that is not
 * 3 or a rotation row that is not 4; a missing named group or noise with S > 0; an input or output tensor of more than 2^31 - 1
 * elements (the kernels index with 32 bits); more than 2^24 - 1 workgroups in one launch.
 * Profiling stages (gsr_profile_*): "densify_plan", "densify_apply".
 */
#ifndef GSR_DENSIFY_H_INCLUDED
#define GSR_DENSIFY_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_DENSIFY_KEEP 0
#define GSR_DENSIFY_PRUNE 1
#define GSR_DENSIFY_CLONE 2
#define GSR_DENSIFY_SPLIT 3
#define GSR_DENSIFY_SPLIT_N 2                          /* children per split row */
#define GSR_DENSIFY_MAX_GROUPS 16
#define GSR_DENSIFY_PLAN_ROWS 1024                     /* rows per workgroup of the plan and of the map */
#define GSR_DENSIFY_SCAN_THREADS 256                   /* workgroup totals the scan takes per loop iteration */
#define GSR_DENSIFY_LOG_SHRINK 0.47000362924573558     /* log(1.6): the children's scales are the parent's / (0.8 * 2) */

size_t gsr_densify_scratch_bytes(int P);               /* 0 for a size that is not valid */
int gsr_densify_plan(int P, const uint8_t* action, void* scratch, int32_t* totals /* [4] on the device */, void* stream);

typedef struct gsr_densify_group {
    const void* param;                          /* [P][row] */
    const void *exp_avg, *exp_avg_sq;           /* [P][row], or both NULL */
    void* out_param;                            /* [P'][row] */
    void *out_exp_avg, *out_exp_avg_sq;         /* [P'][row]; needed where the group has moments */
    int32_t row;                                /* 4-byte words per row, >= 0 */
    int32_t zero_new;                           /* new rows get +0.0 instead of a copy */
} gsr_densify_group;

typedef struct gsr_densify_args {
    int P, K, C, S;                             /* K, C, S as the plan counted them */
    int ngroups;
    int xyz_group, scale_group, rotation_group; /* indices into groups; -1 where S = 0 */
    const gsr_densify_group* groups;            /* host array of ngroups */
    const uint8_t* action;                      /* [P] on the device */
    const void* scratch;                        /* as gsr_densify_plan left it */
    const float* noise;                         /* [2 S][3] on the device; NULL where S = 0 */
    int32_t* src_of;                            /* [P'] on the device, scratch */
    void* stream;
} gsr_densify_args;

int gsr_densify_apply(const gsr_densify_args* args);
#ifdef __cplusplus
}
#endif
#endif /* GSR_DENSIFY_H_INCLUDED */
