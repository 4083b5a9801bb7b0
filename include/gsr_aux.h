/*
 * gsr_aux.h -- depth and alpha maps of libgsr_hip.so (include/gsr.h), from the same blend pass as the colour.
 * Entry points beside the core ABI of gsr.h, whose declarations and struct layouts they leave as they are.
 */
#ifndef GSR_AUX_H_INCLUDED
#define GSR_AUX_H_INCLUDED
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
/*
 * Depth and alpha maps (opt-in; no reference counterpart).  The same forward and backward, with two more per-pixel outputs
 * accumulated in the same blend pass:
 *   D(p) = sum_i v_i alpha_i T_i(p)  over exactly the (pixel, Gaussian) pairs that blend into the colour, no background term;
 *   A(p) = 1 - T_final(p)            (T_final: the image state's final_T).
 * v_i is the view-space depth z_i the geometry kernel sorts by (GSR_AUX_DEPTH) or 1 / z_i (GSR_AUX_INVDEPTH).  Every output of
 * the default calls -- image, radii, the state buffers' contents -- is bit-identical with these variants; they run kernels of their
 * own.  The backward takes dL/dD and dL/dA (either may be NULL = zero) on top of dL_dpix; both flow into every input gradient
 * through dL/dalpha_i, and dL/dv_i = alpha_i T_i dL/dD into dL/dmean3D (dL/dxyz in leaf mode) along the view-space z axis.
 * A call sequence is all-aux or all-default: gsr_forward_preprocess*_aux (the splat records carry v_i), gsr_forward_render_aux,
 * gsr_backward_blend_aux, gsr_backward_gaussians_aux, all with the same mode and scratch.
 */
#define GSR_AUX_DEPTH    1   /* v_i = z_i */
#define GSR_AUX_INVDEPTH 2   /* v_i = 1 / z_i */
typedef struct {
	int mode;                /* GSR_AUX_DEPTH or GSR_AUX_INVDEPTH (preprocess reads nothing else) */
	float* out_depth;        /* [H][W] D, fully written by gsr_forward_render_aux (0 where nothing blends) */
	float* out_alpha;        /* [H][W] A, fully written by gsr_forward_render_aux */
	const float* dL_ddepth;  /* [H][W] or NULL: backward input */
	const float* dL_dalpha;  /* [H][W] or NULL: backward input */
	void* scratch;           /* gsr_aux_bytes(num_rendered, W, H) bytes, 16-byte aligned: written by the forward (render), read by the
	                            backward blend -- it travels forward -> backward like the image state */
} gsr_aux_args;
typedef struct {
	size_t ckpt_depth;       /* [R / 512 + 2][256] f32: per-pixel D beside every depth checkpoint of a heavy tile (gsr_binning_layout.checkpoints) */
	size_t final_D;          /* [W*H] f32: D of the pixels of heavy tiles (the backward's depth segments restart from it) */
	size_t total;
} gsr_aux_layout;
int gsr_aux_layout_of(int64_t num_rendered, int width, int height, gsr_aux_layout* out);
size_t gsr_aux_bytes(int64_t num_rendered, int width, int height);
int gsr_forward_preprocess_aux(
	const gsr_aux_args* aux,
	int P, int D, int M, int width, int height,
	const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
	const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
	const float* viewmatrix, const float* projmatrix, const float* cam_pos,
	float tan_fovx, float tan_fovy, int prefiltered,
	int* radii, void* geometry, int64_t* num_rendered_host, void* stream, int debug);
int gsr_forward_preprocess_leaf_aux(
	const gsr_aux_args* aux,
	int P, int D, int M, int width, int height,
	const float* xyz, const float* features_dc, const float* features_rest,
	const float* opacity_logits, const float* log_scales, float scale_modifier, const float* raw_rotations,
	const float* viewmatrix, const float* projmatrix, const float* cam_pos,
	float tan_fovx, float tan_fovy, int prefiltered,
	int* radii, void* geometry, int64_t* num_rendered_host, void* stream, int debug);
int gsr_forward_render_aux(
	const gsr_aux_args* aux,
	int P, int64_t num_rendered, int width, int height,
	const float* background, const int* radii,
	void* geometry, void* binning, void* image,
	float* out_color, void* stream, int debug);
int gsr_backward_blend_aux(const gsr_backward_args* args, const gsr_aux_args* aux);
int gsr_backward_gaussians_aux(const gsr_backward_args* args, const gsr_aux_args* aux, int first, int count, int out_row0);
#ifdef __cplusplus
}
#endif
#endif /* GSR_AUX_H_INCLUDED */
