/*
 * gsr_mcmc.h -- the mechanical pieces of fixed-budget training ("3D Gaussian Splatting as Markov Chain Monte Carlo"; gsplat's
 * MCMCStrategy: inject_noise_to_position, relocate / sample_add with compute_relocation, and the opacity and scale regulariser).
 * Entry points beside the core ABI of gsr.h, whose declarations they leave as they are.  The policy -- when to relocate, which rows
 * are dead, which live rows they move onto -- stays with the caller.
 *
 * All float arrays are float32 on the device, laid out as the optimiser's leaves (fused_params): xyz [P][3], opacity logits [P][1],
 * log-scales [P][3], unnormalised quaternions [P][4] as (r, x, y, z).  Indices are int64 on the device.  P < 2^31.
 *
 * gsr_mcmc_noise -- one launch, one thread per Gaussian, no LDS, no atomics:
 *   o = sigmoid(logit),  s = exp(log_scale),  R = R(q / |q|) (the matrix every other kernel of the library builds),
 *   gate = 1 / (1 + exp(-100 ((1 - o) - 0.995))),   xyz += R (s^2 * (R^T (noise * (gate * scaler))))     [= Sigma (noise gate scaler)]
 * noise [P][3] is the caller's standard-normal draw, scaler = noise_lr * lr_xyz.  The gate is evaluated in double precision from the
 * logit (in fp32 its factor of 100 on the opacity costs two digits); where its exponential overflows in fp32 -- an argument above
 * log(FLT_MAX), o above about 0.89 -- the gate is exactly 0, as in an fp32 evaluation, and the row keeps its bits.  No NaN comes out
 * of finite inputs.
 *
 * gsr_mcmc_relocate -- D entries (dst[j], src[j]): row dst[j] of every group becomes a copy of row src[j], and the opacity and the
 * scales of the source and of its copies are recomputed so that the rendered distribution is kept (Eq. 9 of the paper):
 *   n  = min(GSR_MCMC_MAX_RATIO, 1 + the number of entries whose source is src[j])
 *   o  = sigmoid(logit[src[j]]),  o' = 1 - (1 - o)^(1 / n)
 *   denom = sum_{k = 0 .. n - 1} C(n, k + 1) (-1)^k o'^(k + 1) / sqrt(k + 1)
 *           (= sum_{i = 1 .. n} sum_{k = 0 .. i - 1} C(i - 1, k) (-1)^k o'^(k + 1) / sqrt(k + 1), by the hockey-stick identity)
 *   new logit = logit(clamp(o', min_opacity, 1 - 2^-23)),   new log-scales = log((o / denom) exp(log_scale[src[j]]))
 * evaluated in double precision from the float32 leaves and rounded once.  Both new values go to rows src[j] and dst[j] of the
 * opacity and the scale group; in every other group row dst[j] gets the bits of row src[j].  With zero_src_moments both moments of
 * row src[j] of every group that has moments become +0.0; the moments of dst rows are never touched.  groups[k].row is the row
 * length in floats; 0 is allowed (features_rest at SH degree 0) and such a group is skipped.  exp_avg and exp_avg_sq are given
 * together or both NULL.
 * Preconditions, the caller's to keep: dst holds no row twice and no row that src holds.  An entry with an index outside [0, P) is
 * skipped.  Growing the set is the same call: enlarge the tensors (zero moments for the new rows), pass the new rows as dst and
 * zero_src_moments = 0.
 * Three kernels behind a memset of `counts` (P int32, contents irrelevant): count the sources (integer atomic adds, independent of
 * order); one wave per entry reads the source's old values and writes row dst[j] only; one wave per entry copies the new logit and
 * log-scales back to row src[j] (entries with one source write the same bits) and zeroes its moments.  No floating-point atomics:
 * every result is bitwise reproducible.  D = 0 returns GSR_OK and launches nothing.
 *
 * gsr_mcmc_regularizer -- value and gradients in one pass:
 *   val[0] = w_o (1 / P) sum sigmoid(l) + w_s (1 / (3 P)) sum exp(s)
 *   dL_dopacity = (w_o / P) sigmoid(l) sigmoid(-l),   dL_dscaling = (w_s / (3 P)) exp(s)        (each written where not NULL)
 * sigmoid(l) sigmoid(-l) is formed as that product from one exponential of -|l|, so that it keeps its digits where y (1 - y)
 * cancels.  A thread sums at most GSR_MCMC_REG_ELEMS_PER_THREAD terms in index order, a workgroup of GSR_MCMC_REG_THREADS threads
 * adds them as a tree (lanes, then waves), and one workgroup folds the partial sums in `scratch` in a fixed order in double:
 * bitwise reproducible, and with all terms positive within (GSR_MCMC_REG_ELEMS_PER_THREAD + log2(GSR_MCMC_REG_THREADS) + 4) 2^-24
 * of the exact value.  scratch: gsr_mcmc_regularizer_scratch_bytes(P) bytes, contents irrelevant, free for reuse once the call's
 * work on the stream has finished.
 *
 * Refused with GSR_ERR_INVALID_ARGUMENT before any device work, with a message that starts with the function's name: a NULL
 * required pointer; P < 1; D < 0; ngroups outside 1 .. GSR_ADAM_MAX_GROUPS; opacity_group or scale_group that is no group, the two
 * being one group, an opacity group whose row is not 1 or a scale group whose row is not 3; a negative row; one moment without the
 * other; min_opacity outside (0, 1); a tensor of more than 2^31 - 1 elements (the kernels index with 32 bits); more than 2^24 - 1
 * workgroups in one launch.
 * Profiling stages (gsr_profile_*): "mcmc_noise", "mcmc_relocate", "mcmc_reg".
 */
#ifndef GSR_MCMC_H_INCLUDED
#define GSR_MCMC_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_MCMC_MAX_RATIO 51               /* gsplat's n_max */
#define GSR_MCMC_REG_THREADS 256            /* workgroup size of the regulariser */
#define GSR_MCMC_REG_ELEMS_PER_THREAD 12    /* the longest chain a thread sums: 4 Gaussians' 12 scale entries */

int gsr_mcmc_noise(int P, float* xyz, const float* opacity, const float* scaling, const float* rotation, const float* noise,
                   float scaler, void* stream);

typedef struct gsr_mcmc_group {
    float* param;                     /* [P][row] */
    float *exp_avg, *exp_avg_sq;      /* [P][row], or both NULL */
    int32_t row;                      /* floats per row, >= 0 */
} gsr_mcmc_group;

typedef struct gsr_mcmc_relocate_args {
    int P, D, ngroups;
    int opacity_group, scale_group;   /* indices into groups */
    int zero_src_moments;
    float min_opacity;
    const gsr_mcmc_group* groups;     /* host array of ngroups */
    const int64_t *dst, *src;         /* [D] on the device */
    int32_t* counts;                  /* [P] on the device, scratch */
    void* stream;
} gsr_mcmc_relocate_args;

int gsr_mcmc_relocate(const gsr_mcmc_relocate_args* args);

size_t gsr_mcmc_regularizer_scratch_bytes(int P);   /* 0 for a size that is not valid */
int gsr_mcmc_regularizer(int P, const float* opacity, const float* scaling, float w_o, float w_s, float* val,
                         float* dL_dopacity /* or NULL */, float* dL_dscaling /* or NULL */, void* scratch, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* GSR_MCMC_H_INCLUDED */
