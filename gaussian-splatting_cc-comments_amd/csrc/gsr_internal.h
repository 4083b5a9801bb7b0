// gsr_internal.h -- host-side glue shared by the translation units of libgsr_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/gsr.h"
#include "../../include/gsr_aux.h"
#include "../../include/gsr_cam.h"
#include "../../include/gsr_absgrad.h"
#include "../../include/gsr_camera_model.h"
#include "../../include/gsr_cam_cm.h"
#include "gsr_device.h"

#define GSR_PREPROCESS_BLOCK 256  // Gaussians per workgroup of the binning kernels (granularity of their scans)
// The instance count (num_rendered) is accumulated by the preprocess workgroups with one atomic add each,
// spread over this many words so that no address sees more than a few dozen (3 900 adds to ONE word cost
// 9 us of serialisation); the host adds the parts after the read-back.
#define GSR_COUNT_PARTS 64
// status words: [0] prefiltered trap, [2] 1 = the depth sort's result is in the ping-pong partners (perm_alt, depth_keys_alt),
// [3] 1 = slot_base is final and numbers the gradient slots in INDEX order (the bucket depth sort's first kernel did it); 0 = the
// binning numbers them in depth order itself (tilebin.hip pass 1 / the key emission),
// [4, 68) partial instance counts, [68, 132) partial maxima of ~depth_key, [132, 196) partial maxima of depth_key
// (visible Gaussians only; the depth sort orders key - min, so only the bits of max - min need passes)
#define GSR_STATUS_NEGMIN (4 + GSR_COUNT_PARTS)
#define GSR_STATUS_MAX (4 + 2 * GSR_COUNT_PARTS)
#define GSR_STATUS_WORDS (4 + 3 * GSR_COUNT_PARTS)

// A Gaussian's run of per-tile gradient slots is added by its own lane up to this length and by the whole wave beyond it, in
// gaussian_backward.hip (gsr_add_slot) and in absgrad.hip alike.
#ifndef GSR_SLOT_COOP
#define GSR_SLOT_COOP 30   // swept on MI355X at C3: 12 / 18 / 24 / 36 -> 0.172 / 0.164 / 0.166 / 0.171 ms with the slots in depth order (round 2);
                           // in index order (round 4) a lane's records lie next to its neighbours': 18 / 30 / 58 -> 0.130 / 0.120 / 0.118 ms at C3,
                           // 0.745 / 0.626 / 0.628 at C5 (the per-Gaussian backward)
#endif

static inline size_t gsr_align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }
static inline int gsr_grid_x(int W) { return (W + GSR_TILE_X - 1) / GSR_TILE_X; }
static inline int gsr_grid_y(int H) { return (H + GSR_TILE_Y - 1) / GSR_TILE_Y; }

// Typed views of the opaque blobs (offsets published through gsr_*_layout_of()).
struct GsrGeometry {
	GsrSplat* splat;
	uint32_t* depth_keys;      // depth bits per Gaussian (0xFFFFFFFF = culled); after the depth sort: sorted keys
	uint32_t* depth_keys_alt;  // ping-pong partner
	uint32_t* perm;            // identity; after the depth sort: Gaussian ids in (depth, id) order
	uint32_t* perm_alt;
	uint32_t* tiles_touched;
	uint2* rect;               // dense copy of the tile rectangle {x | y << 16, w | h << 16}: what the depth-ordered kernels gather
	uint2* rshape;             // {rectangle in one word, trim word} (gsr_rect_trim.h): what the depth sort carries along and the column-pair binning reads
	uint32_t* slot_base;       // first (Gaussian,tile) gradient slot: exclusive prefix of tiles_touched in index order (final once status word 3 is set)
	uint8_t* clamped;
	float* sh_ddir;            // [9][P] d(colour channel c)/d(unit view direction) of the visible Gaussians (plane 3c + {x,y,z})
	uint32_t* status;             // GSR_STATUS_* words

	uint32_t* sorted_block_sums;  // per-workgroup tile counts in depth order (the key emission takes their prefix sums itself)
	uint32_t* block_tiles;        // tile counts of the preprocess kernel's workgroups (256 Gaussians each, index order): slot_base's prefix
	void* sort_table;             // radix histogram table for the P-sized depth sort
	void* col_table;              // tilebin.hip, pass 1 (column pairs by tile column): chunk sums, block rows, digit totals
};

// Depth checkpoints of heavy tiles (lists of at least 2 * GSR_CKPT_STRIDE instances): every GSR_CKPT_STRIDE instances the forward
// blend stores each pixel's running (T, C) BEFORE the instance at that position; the backward blend can then start in the middle
// of a list (render_backward.hip).  One 4-KB record (256 pixels x float4) per checkpoint, indexed by the checkpoint's position in the
// global sorted instance list: record (range.x + p) / GSR_CKPT_STRIDE for local position p -- tiles own disjoint ranges and only
// tiles of at least two strides store any, so no two checkpoints share a record.
#ifndef GSR_CKPT_STRIDE
#define GSR_CKPT_STRIDE 512    // (1024 until the lists were trimmed: gsr_rect_trim.h -- a list position now holds a contributor 1.6 x as often)
#endif
#ifndef GSR_SPLIT_MIN_LIST
#define GSR_SPLIT_MIN_LIST 640 // forward: shortest list that is handed out as four band waves (1024 until the lists were trimmed)
#endif
#define GSR_CKPT_MAX_SEGMENTS 15   // segments a heavy tile's walk is cut into at most (4 bits of the dispatch entry, 0 = whole tile)
static inline size_t gsr_checkpoint_records(int64_t R) { return (size_t)(R / GSR_CKPT_STRIDE) + 2; }

struct GsrImage {
	float* final_C;            // [3][W*H] accumulated colour without the background term (heavy tiles only: the backward's segments need it)
	float* final_T;
	uint32_t* n_contrib;
	uint2* ranges;
	uint32_t* tile_max_contrib;
	uint32_t* tile_order;      // tiles in descending order of backward work (longest-processing-time-first dispatch)
};

struct GsrBinning {
	uint32_t* point_list;      // sorted Gaussian ids (final)
	uint32_t* point_list_alt;  // ping-pong partner
	uint32_t* tile_keys;       // sorted tile ids (final)
	uint32_t* tile_keys_alt;   // after the forward: [R] validity BYTES of the backward's gradient slots (zeroed by tile_ranges)
	uint8_t* band_masks;       // [R] bytes inside tile_keys_alt, behind the validity bytes: gsr_tile_band_mask of every list position the forward
	                           // blend staged, for the backward blend (render_forward.hip / render_backward.hip)
	void* sort_table;          // radix histogram table for the R-sized tile sort
	float4* checkpoints;      // [gsr_checkpoint_records(R)][256] depth checkpoints of heavy tiles (see GSR_CKPT_STRIDE)
};

// Per-call pointers of the depth-and-alpha variants of the blend kernels (include/gsr.h gsr_aux_args)
struct GsrAuxBlend {
	float* out_depth;          // [W*H] forward outputs
	float* out_alpha;
	float* ckpt_depth;         // [gsr_checkpoint_records(R)][256] per-pixel D beside each (T, C) checkpoint
	float* final_D;            // [W*H] D of heavy tiles' pixels (as final_C)
	const float* dL_ddepth;    // [W*H] backward inputs, NULL = zero
	const float* dL_dalpha;
};

GsrGeometry gsr_geometry_view(void* blob, int P);
GsrImage gsr_image_view(void* blob, int W, int H);
GsrBinning gsr_binning_view(void* blob, int P, int64_t R, int W, int H);

// The state of one forward as every call after stage 1 sees it, checked and opened in one place (api.hip, gsr_frame_open).  img is
// zero when the call reads no image, bin and slot_valid when nothing was rendered (R == 0), slots when the call takes none.
struct GsrFrame {
	int P, W, H;
	int64_t R;
	GsrGeometry g;
	GsrImage img;
	GsrBinning bin;
	GsrGradSlot* slots;
	// Validity bytes of the gradient slots: the tile sort's dead ping-pong buffer, cleared at the end of the forward.
	// Which slots get written depends on the forward alone (not on dL_dpix), so a second backward over the
	// same forward state (retain_graph) finds exactly the bytes it would set itself.
	uint8_t* slot_valid;
	hipStream_t s;
	int debug;
	bool cull;   // !GSR_DEBUG_NO_CULL
};

// The camera-gradient target of the per-Gaussian backward: the kernels also store one row of 32 floats per wave of 64 Gaussians in
// `rows` (gsr_cam_rows(count) rows; first must be 0), and a fold adds the rows into the outputs -- without a camera model the 35 of
// include/gsr_cam.h (dL_dmid = dL_dprojmatrix), under one the 16 + 4 + 3 of include/gsr_cam_cm.h (dL_dmid = dL_dintrinsics)
struct GsrCamTarget {
	float* rows;
	float* dL_dviewmatrix;
	float* dL_dmid;
	float* dL_dcampos;
};

// What the per-Gaussian passes (stage 1 and the per-Gaussian backward) run with beyond their arguments, checked and built in one place
// (api.hip, gsr_gaussian_options).
struct GsrGaussianOptions {
	int aux = 0;                             // 0, or the depth-and-alpha mode (GSR_AUX_*): stage 1 also stores the depth value v in the splat record's last
	                                         // word; the backward sums the slots' tenth word (dL/dv) and chains it into dL/dmean3D
	int aa = 0;                              // the anti-aliased path (include/gsr_aa.h): the record's opacity is opacity * rho (gsr_aa.h) ...
	const float* aa_opacities = nullptr;     // ... and the backward's opacity input: dL/dopacity = dL/dopacity_record * rho, and dL/drho into dL/dcov3D and dL/dmean3D
	const gsr_camera_model* cm = nullptr;    // NULL, or the camera-model kernels (include/gsr_camera_model.h), with focal_x / focal_y = fx, fy
	GsrCamTarget cam = {};                   // rows == NULL: no camera gradients
};

// error plumbing (api.hip)
int gsr_fail(int code, const char* fmt, ...);
int gsr_check_hip(hipError_t e, const char* what);
// Called after each stage: in debug mode synchronises the stream and reports kernel errors.
int gsr_stage_done(hipStream_t s, int debug, const char* stage);
// Per-kernel event profiling (api.hip); no-ops unless gsr_profile_begin() was called for this stream.
void gsr_prof_mark_begin(hipStream_t s, const char* name);
void gsr_prof_mark_end(hipStream_t s);
bool gsr_prof_kernel_events(hipStream_t s, const char* name, hipEvent_t* a, hipEvent_t* b);

struct GsrProfScope {
	hipStream_t s;
	GsrProfScope(hipStream_t st, const char* name) : s(st) { gsr_prof_mark_begin(s, name); }
	~GsrProfScope() { gsr_prof_mark_end(s); }
};

// ---- kernel launchers ------------------------------------------------------------------------
// The one launch call of every kernel that may carry events.  start / stop: optional events that the kernel's own dispatch packet
// signals (hipExtLaunchKernelGGL) -- its timestamps, or "this kernel has finished" for another stream to wait on.  A hipEventRecord
// in front of or behind the kernel would be a barrier packet of its own and costs the stream's next launch 6-8 us.  Without an event
// it is the plain launch.  The arguments are converted to the kernel's own parameter types here (the Ext call packs them as given).
template <typename T> struct GsrSame { typedef T type; };
template <typename... P>
static inline void gsr_launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, hipEvent_t start, hipEvent_t stop,
                              typename GsrSame<P>::type... args)
{
	if (start || stop) hipExtLaunchKernelGGL(kernel, grid, block, lds, s, start, stop, 0, args...);
	else hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
}

// The one place where a call's run-time variant becomes template arguments: f(LEAF, AUX, AA) is called with the three as
// std::integral_constant values (LEAF() etc. are constant expressions).  aux: 0 or a GSR_AUX_* mode; a kernel without one of the
// three variants ignores that argument (the colour kernel has no AA form, the blend kernels only "maps or not").  The order of the
// branches is the order in which a file's instantiations appear in its device code (`make audit` output is compared across commits).
template <typename F>
static inline void gsr_variant(bool leaf, int aux, bool aa, F&& f)
{
	auto with_leaf = [&](auto AUX, auto AA) {
		if (leaf) f(std::true_type{}, AUX, AA);
		else f(std::false_type{}, AUX, AA);
	};
	auto with_aux = [&](auto AA) {
		if (aux == GSR_AUX_INVDEPTH) with_leaf(std::integral_constant<int, GSR_AUX_INVDEPTH>{}, AA);
		else if (aux) with_leaf(std::integral_constant<int, GSR_AUX_DEPTH>{}, AA);
		else with_leaf(std::integral_constant<int, 0>{}, AA);
	};
	if (aa) with_aux(std::true_type{});
	else with_aux(std::false_type{});
}

struct GsrPreprocessArgs {
	int P, D, M, W, H;
	const float* means3D;
	const float* shs;
	const float* colors_precomp;
	const float* opacities;
	const float* scales;
	float scale_modifier;
	const float* rotations;
	const float* cov3D_precomp;
	const float* viewmatrix;
	const float* projmatrix;
	const float* cam_pos;
	float tan_fovx, tan_fovy, focal_x, focal_y;
	int prefiltered;
	int trim;   // 0: GSR_DEBUG_NO_TRIM
	int* radii;
	GsrGeometry g;
	// leaf mode (gsr_forward_preprocess_leaf): shs = _features_dc, shs_rest = _features_rest,
	// opacities / scales / rotations are the raw leaves and are activated inside the kernel
	int leaf;
	const float* shs_rest;
};

// preprocess.hip
// done: NULL, or an event signalled when the kernel has finished (gsr_launch); the colour kernel has no anti-aliased variant
void gsr_launch_preprocess(const GsrPreprocessArgs& a, hipStream_t s, hipEvent_t done, const GsrGaussianOptions& o);
void gsr_launch_zero_status(uint32_t* status, hipStream_t s, hipEvent_t done);
bool gsr_preprocess_needs_color(const GsrPreprocessArgs& a);
void gsr_launch_preprocess_color(const GsrPreprocessArgs& a, hipStream_t s, int wgs_per_cu, int aux);
void gsr_launch_mark_visible(int P, const float* means3D, const float* viewmatrix, uint8_t* present, hipStream_t s);

// binning.hip
void gsr_launch_sorted_block_sums(GsrGeometry g, int P, int result_in_alt, hipStream_t s);
void gsr_launch_duplicate_keys(GsrGeometry g, int P, int W, void* keys, int key_bytes, uint32_t* vals, uint32_t* clear, size_t clear_words, hipStream_t s);
void gsr_launch_tile_ranges(const void* tile_keys, int key_bytes, int64_t R, uint2* ranges, int ntiles, uint32_t* valid, hipStream_t s);
void gsr_launch_tile_order(GsrImage img, int ntiles, bool backward, int64_t num_rendered, bool split, hipStream_t s, bool normalise_empty = false);
uint32_t gsr_tile_order_max_split(int ntiles);      // forward: tiles that may be split into four band entries
uint32_t gsr_tile_order_max_segments(int ntiles);   // backward: extra entries for the depth segments of heavy tiles

// tilebin.hip: the sorted instance list by column pairs (images of at most 256 x 256 tiles)
bool gsr_tilebin_applies(int W, int H);
size_t gsr_tilebin_col_clear_words(size_t P);   // leading words of col_table that the preprocess kernel zeroes
size_t gsr_tilebin_col_table_bytes(size_t P);
size_t gsr_tilebin_row_clear_words(size_t R);
size_t gsr_tilebin_row_table_bytes(size_t R);
void gsr_launch_tilebin_col_hist(GsrGeometry g, int P, int result_in_alt, hipStream_t s, bool seg_ready = false);
uint4* gsr_tilebin_seg(GsrGeometry g, int P);
uint4* gsr_tilebin_recs(GsrGeometry g, int P);
void gsr_launch_tilebin_col_scatter(GsrGeometry g, int P, GsrBinning b, int64_t R, hipStream_t s);
void gsr_launch_tilebin_row_hist(GsrGeometry g, int P, GsrBinning b, int64_t R, hipStream_t s);
void gsr_launch_tilebin_row_scatter(GsrGeometry g, int P, GsrBinning b, int64_t R, uint2* ranges, int W, int H, hipStream_t s);

// sort.hip
int gsr_radix_num_passes(int nbits_total);
size_t gsr_radix_table_bytes(size_t n);
size_t gsr_radix_clear_words(size_t n);  // leading words of the table that the producer of the keys must zero
void gsr_launch_slot_base_finish(uint32_t* slot_base, const uint32_t* block_tiles, uint32_t* status, size_t n, hipStream_t s);
void gsr_radix_sort_passes(void* k0, uint32_t* v0, void* k1, uint32_t* v1, size_t n, int nbits_total, int npass_total,
                           int pass_first, int pass_count, void* table_mem, const uint32_t* bias, int key_bytes, hipStream_t s);
void gsr_radix_sort_u32(void* k0, uint32_t* v0, void* k1, uint32_t* v1, size_t n, int nbits_total, void* table_mem,
                        int* result_in_first, int clear_table, int key_bytes, hipStream_t s);
void gsr_radix_top_pass(const uint32_t* k0, uint32_t* k1, const uint2* rec_in, uint4* rec_out, size_t n, void* table_mem, const uint32_t* bias, hipStream_t s,
                        uint32_t* slot_base, const uint32_t* block_tiles, uint32_t* status);
int gsr_radix_top_chunks(size_t n);
// depthsort.hip: depth order in three launches (top-digit buckets, then every bucket sorted inside LDS) for up to this many Gaussians
#ifndef GSR_BUCKET_SORT_MAX_P
#define GSR_BUCKET_SORT_MAX_P (2 << 20)
#endif
bool gsr_bucket_sort_applies(int P);
void gsr_launch_depth_bucket_sort(GsrGeometry g, int P, uint4* seg, hipStream_t s);
// bytes per tile key of an instance-sized sort: 2 when every tile id fits 16 bits AND the sort runs the instance-sized
// kernels (sort.hip), else 4
int gsr_tile_key_bytes(int ntiles, size_t num_rendered);

// render_forward.hip
// ordered: tile_order holds ntiles + 3 * gsr_tile_order_max_split(ntiles) entries; aux: NULL, or the depth-and-alpha variant
void gsr_launch_render_forward(const GsrFrame& f, const float* bg, float* out_color, bool ordered, const GsrAuxBlend* aux);

// render_backward.hip
// t_*: NULL, or taken by the kernel's own dispatch packet (gsr_launch); aux: NULL, or the depth-and-alpha variant
// absgrad: the ABS variant, which also fills the slots' words 10 and 11 (include/gsr_absgrad.h)
void gsr_launch_render_backward(const GsrFrame& f, const float* bg, const float* dL_dpix, hipEvent_t t_start, hipEvent_t t_stop,
                                const GsrAuxBlend* aux, bool absgrad);

// absgrad.hip: per-Gaussian fold of the slots' words 10 and 11 (include/gsr_absgrad.h) for the Gaussians [first, first + count).
// radii: NULL = visibility from tiles_touched; the frame's slot_valid: NULL when nothing was rendered (every Gaussian then gets zeros)
void gsr_launch_absgrad_fold(const GsrFrame& f, int first, int count, const int* radii, float* abs_dL_dmean2D, float* stat_abs_gradient_accum);

// contrib.hip: blend-weight statistics (include/gsr_contrib.h).  scratch: R 16-byte records, then (at gsr_contrib_valid_offset) R validity
// bytes, which gsr_contributions clears on the stream before the tile pass
size_t gsr_contrib_valid_offset(int64_t R);
void gsr_launch_contrib_tiles(const GsrFrame& f, const float* pixel_weight, void* scratch);
void gsr_launch_contrib_gaussians(const GsrFrame& f, const void* scratch, float* weight_sum, float* weight_max, int32_t* pixel_count);

// features.hip: K blended feature channels and their gradients (include/gsr_features.h).  scratch: gsr_features_chunks(K) x R 16-byte
// records, then (at gsr_features_valid_offset) R validity bytes, which gsr_features_backward clears on the stream before the tile pass.
// the frame's slots: NULL (into_slots = 0), or the gradient slots whose words 0..5 the tile pass adds into
int gsr_features_chunks(int K);
size_t gsr_features_valid_offset(int64_t R, int K);
void gsr_launch_features_forward(const GsrFrame& f, int K, const float* features, float* out);
void gsr_launch_features_backward_tiles(const GsrFrame& f, int K, const float* features, const float* dL_dout, void* scratch);
void gsr_launch_features_fold(const GsrFrame& f, int K, const void* scratch, float* dL_dfeatures);

// distortion.hip: the depth-distortion map of an aux-mode forward and its gradient (include/gsr_distortion.h).  state: the planes A, mu,
// S [3][H][W]; the backward adds into words 0..5 and 9 of the frame's gradient slots
void gsr_launch_distortion_forward(const GsrFrame& f, float* out, float* state);
void gsr_launch_distortion_backward(const GsrFrame& f, const float* state, const float* dL_ddist);

// median.hip: the median-depth map, the per-pixel index maps and the median depth's gradient (include/gsr_median.h).  Outputs: NULL =
// not wanted; state: the median's list position per pixel [H][W]; the backward adds into word 9 of the frame's gradient slots
void gsr_launch_median_forward(const GsrFrame& f, float* out_depth, int32_t* out_median, int32_t* out_dominant, float* out_weight,
                               uint32_t* state, bool full_walk);
void gsr_launch_median_backward(const GsrFrame& f, const uint32_t* state, const float* dL_dmedian);

// gaussian_backward.hip
struct GsrGaussianBackwardArgs {
	int P, D, M, W, H;
	int first, count;          // the Gaussians [first, first + count) are processed (first is a multiple of 64)
	int out_row0;              // gradient outputs are written at row (index - out_row0): 0, or `first` for per-part buffers
	const float* means3D;
	const float* shs;
	const float* colors_precomp;
	const float* scales;
	float scale_modifier;
	const float* rotations;
	const float* cov3D_precomp;
	const float* viewmatrix;
	const float* projmatrix;
	const float* cam_pos;
	float tan_fovx, tan_fovy, focal_x, focal_y;
	const int* radii;          // may be NULL: visibility is then taken from tiles_touched (same predicate)
	GsrGeometry g;
	const GsrGradSlot* slots;
	const uint8_t* slot_valid;
	float* dL_dmean2D;
	float* dL_dconic;
	float* dL_dopacity;
	float* dL_dcolor;
	float* dL_dmean3D;
	float* dL_dcov3D;
	float* dL_dsh;
	float* dL_dscale;
	float* dL_drot;
	// leaf mode (gsr_backward_leaf): inputs as in GsrPreprocessArgs; dL_dsh = grad of _features_dc,
	// dL_dsh_rest = grad of _features_rest, dL_dopacity/dL_dscale/dL_drot are gradients w.r.t. the raw
	// leaves; dL_dconic, dL_dcolor, dL_dcov3D may be NULL (not written)
	int leaf;
	const float* shs_rest;
	float* dL_dsh_rest;
	// densification statistics (train.py:157-159, scene/gaussian_model.py:599-602), each may be NULL
	float* stat_xyz_gradient_accum;  // [P] += ||dL_dmean2D.xy|| for visible Gaussians
	float* stat_denom;               // [P] += 1 for visible Gaussians
	float* stat_max_radii2D;         // [P] = max(itself, radius) for visible Gaussians
};
// the anti-aliased path (include/gsr_aa.h): the opacity INPUT (activated; the logit in leaf mode), which the record no longer holds --
// it holds opacity * rho.  A struct of its own so that the default kernels' arguments keep their layout.
struct GsrGaussianBackwardArgsAA : GsrGaussianBackwardArgs {
	const float* opacities;
};
void gsr_launch_gaussian_backward(const GsrGaussianBackwardArgs& a, hipStream_t s, const GsrGaussianOptions& o);
size_t gsr_cam_rows(int P);
void gsr_launch_camera_grad_fold(const float* partials, int nrows, float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos, hipStream_t s);
void gsr_launch_cam_cm_fold(const float* partials, int nrows, float* dL_dviewmatrix, float* dL_dintrinsics, float* dL_dcampos, hipStream_t s);
void gsr_launch_sh_grad_from_views(int P, int D, int M, int V, const float* means3D, const float* cam_pos, const float* dL_dRGB,
                                   int64_t view_stride, float* dL_dsh, hipStream_t s);

// loss.hip
size_t gsr_loss_scratch_layout(int C, int H, int W, size_t* maps_off, size_t* partial_off, int* ntiles);
void gsr_launch_l1_ssim(int C, int H, int W, const float* img, const float* gt, float lambda, float* loss_out, float* dL_dimg,
                        void* scratch, hipStream_t s);

// loss_ext.hip: the same loss with a pixel mask, an exposure and an inverse-depth term (include/gsr_loss_ext.h)
struct gsr_loss_ext_args;
size_t gsr_loss_ext_scratch_layout(int C, int H, int W, size_t* maps_off, size_t* partial_off, size_t* epart_off, int* ntiles, int* ntiles_xy);
void gsr_launch_l1_ssim_ext(const gsr_loss_ext_args& a, hipStream_t s);

// bilagrid.hip: the bilateral grid of affine colour transforms (include/gsr_bilagrid.h)
struct gsr_bilagrid_args;
long long gsr_bilagrid_tiles(int H, int W);                           // workgroups of the slice kernels
long long gsr_bilagrid_gather_blocks(int H, int L, int GH, int GW);   // workgroups of the dL_dgrid gather
size_t gsr_bilagrid_scratch_size(int H, int W, int L, int GH, int GW);
size_t gsr_bilagrid_tv_scratch_size(int N, int L, int GH, int GW);
void gsr_launch_bilagrid_slice(const gsr_bilagrid_args& a, hipStream_t s);
void gsr_launch_bilagrid_backward(const gsr_bilagrid_args& a, hipStream_t s);
void gsr_launch_bilagrid_tv(int N, int L, int GH, int GW, const float* grids, float* val, float* dL_dgrids, void* scratch, hipStream_t s);

// mcmc.hip: noise injection, relocation and the regulariser of fixed-budget training (include/gsr_mcmc.h)
struct gsr_mcmc_relocate_args;
long long gsr_mcmc_relocate_blocks(int D);   // workgroups of the per-entry launches
size_t gsr_mcmc_reg_scratch_size(int P);
void gsr_launch_mcmc_noise(int P, float* xyz, const float* opacity, const float* scaling, const float* rotation, const float* noise, float scaler,
                           hipStream_t s);
int gsr_launch_mcmc_relocate(const gsr_mcmc_relocate_args& a, hipStream_t s);   // GSR_OK, or the code of a failed memset
void gsr_launch_mcmc_regularizer(int P, const float* opacity, const float* scaling, float w_o, float w_s, float* val, float* dL_dopacity,
                                 float* dL_dscaling, void* scratch, hipStream_t s);

// densify.hip: clone, split and prune as one compaction (include/gsr_densify.h)
struct gsr_densify_args;
long long gsr_densify_plan_blocks(int P);             // workgroups of the count and the map launch
long long gsr_densify_copy_blocks(long long words);   // workgroups of one group's copy launch
size_t gsr_densify_scratch_size(int P);
void gsr_launch_densify_plan(int P, const uint8_t* action, void* scratch, int32_t* totals, hipStream_t s);
void gsr_launch_densify_apply(const gsr_densify_args& a, hipStream_t s);

// filter3d.hip: Mip-Splatting's 3D smoothing filter (include/gsr_filter3d.h)
struct gsr_filter3d_camera;
size_t gsr_filter3d_scratch_size(int P);
void gsr_launch_filter3d_sweep(int P, int C, const float* xyz, const gsr_filter3d_camera* cameras, int per_camera, float* filter, void* scratch,
                               hipStream_t s);
void gsr_launch_filter3d_activate(int P, const float* opacity, const float* scaling, const float* filter, float* out_o, float* out_s, int baked,
                                  hipStream_t s);   // baked: logit(opacities) and log(scales)
void gsr_launch_filter3d_activate_backward(int P, const float* opacity, const float* scaling, const float* filter, const float* g_opacities,
                                           const float* g_scales, float* d_opacity, float* d_scaling, hipStream_t s);
void gsr_launch_filter3d_reset(int P, float* opacity, const float* scaling, const float* filter, double max_opacity, float* exp_avg, float* exp_avg_sq,
                               hipStream_t s);

// slice4d.hip: 4D Gaussians at a time stamp, the slice and the harmonic colour coefficients (include/gsr_slice4d.h)
struct gsr_slice4d_backward_args {
	int P;
	const float *xyz, *t, *scaling, *scaling_t, *rotation, *rotation_r, *opacity;
	double time, modifier, cutoff;
	const float *g_means3D, *g_cov3D, *g_opacities, *g_velocity;   // any may be NULL: zero
	float *d_xyz, *d_t, *d_scaling, *d_scaling_t, *d_rotation, *d_rotation_r, *d_opacity;   // any may be NULL: not written
};
void gsr_launch_slice4d_forward(int P, const float* xyz, const float* t, const float* scaling, const float* scaling_t, const float* rotation,
                                const float* rotation_r, const float* opacity, double time, double modifier, double cutoff, float* means3D,
                                float* cov3D, float* opacities, float* velocity, hipStream_t s);
void gsr_launch_slice4d_backward(const gsr_slice4d_backward_args& a, hipStream_t s);
void gsr_launch_harmonic_forward(int P, int N, int M, const float* features_t, const float* t, double time, double period, float* shs, hipStream_t s);
void gsr_launch_harmonic_backward(int P, int N, int M, const float* features_t, const float* t, double time, double period, const float* g_shs,
                                  float* d_features_t, float* d_t, hipStream_t s);

// tsdf.hip: TSDF fusion of depth maps and marching tetrahedra (include/gsr_tsdf.h)
struct gsr_tsdf_grid;
struct gsr_tsdf_mesh_plan_t;
size_t gsr_tsdf_mesh_scratch_size(long long nodes);
long long gsr_tsdf_integrate_blocks(const gsr_tsdf_grid& g);
void gsr_launch_tsdf_integrate(const gsr_tsdf_grid& g, float* wsum, float* dsum, float* csum, int C, const gsr_filter3d_camera* cameras, int H, int W,
                               const float* depth, const float* color, const float* weight, float sdf_trunc, float depth_trunc, hipStream_t s);
hipError_t gsr_launch_tsdf_mesh_plan(const gsr_tsdf_grid& g, const float* wsum, const float* dsum, float min_weight, void* scratch, long long totals[2],
                                     hipStream_t s);   // synchronises the stream: totals = {V, F} on the host
void gsr_launch_tsdf_mesh_emit(const gsr_tsdf_mesh_plan_t& plan, const float* csum, float* vertices, float* colors, int32_t* faces, hipStream_t s);

// normals.hip: per-Gaussian normals, depth normals and the normal-consistency loss (include/gsr_normals.h).  world: 0 = view-space output
void gsr_launch_gaussian_normals(int P, const float* scales, const float* rotations, const float* means3D, const float* viewmatrix, int world,
                                 float* out, hipStream_t s);
void gsr_launch_gaussian_normals_backward(int P, const float* scales, const float* rotations, const float* means3D, const float* viewmatrix,
                                          int world, const float* dL_dout, float* dL_drot, hipStream_t s);
size_t gsr_normals_scratch_size(int W, int H);
void gsr_launch_depth_normals(int W, int H, const float* depth, float tanfovx, float tanfovy, float* out, hipStream_t s);
void gsr_launch_depth_normals_backward(int W, int H, const float* depth, float tanfovx, float tanfovy, const float* dL_dout, float* dL_ddepth,
                                       hipStream_t s);
void gsr_launch_normal_consistency_loss(int W, int H, const float* normal_map, const float* depth, const float* alpha, float tanfovx,
                                        float tanfovy, float* vals, float* dL_dnormal, float* dL_ddepth, void* scratch, hipStream_t s);

// optimizer.hip
int gsr_launch_adam(int ngroups, const gsr_adam_group* groups, double beta1, double beta2, double eps, const int* radii, hipStream_t s);

// knn.hip
size_t gsr_knn_scratch_size(int P);
void gsr_launch_knn(int P, const float* points, float* mean_dist2, void* scratch, hipStream_t s);
// knn_graph.hip
size_t gsr_knn_search_scratch_size(int P, int Q);
void gsr_launch_knn_search(int P, const float* points, int Q, const float* queries, int K, float* dist2, int* idx, void* scratch, hipStream_t s);
size_t gsr_knn_graph_scratch_size(int E, int P);
void gsr_launch_knn_graph_build(int E, const int* idx, int P, int* offsets, int* edges, int* num_valid, void* scratch, hipStream_t s);
void gsr_launch_knn_gather(int64_t E, int C, const float* x, const int* idx, float* out, hipStream_t s);
void gsr_launch_knn_gather_backward(int P, int C, const int* offsets, const int* edges, const float* grad_out, float* grad_x, hipStream_t s);
// vq.hip: nearest-code search and centroid update (include/gsr_vq.h)
size_t gsr_vq_assign_scratch_size(int N, int D, int K);
void gsr_launch_vq_assign(int N, int D, const float* x, int K, const float* codebook, int* idx, float* dist2, void* scratch, hipStream_t s);
void gsr_launch_vq_update(int D, const float* x, const float* weight, int K, const int* offsets, const int* members, float* codebook, int* count,
                          float* wsum, hipStream_t s);
// rigidity.hip
size_t gsr_rigidity_scratch_size(int P, int K);
void gsr_launch_rigidity_zero(int P, float* values, float* grad_xyz, float* grad_rot, hipStream_t s);
void gsr_launch_rigidity_loss(int P, int K, const float* xyz, const float* rotation, const int* idx, const float* prev_offset, const float* prev_dist,
                              const float* weight, const float* prev_inv_rot, const int* offsets, const int* edges, float w_rigid, float w_rot, float w_iso,
                              float* values, float* grad_xyz, float* grad_rot, void* scratch, hipStream_t s);
