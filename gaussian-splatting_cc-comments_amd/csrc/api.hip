// api.hip -- the C ABI of libgsr_hip.so (include/gsr.h): buffer layouts, stage orchestration,
// error reporting.  Orchestration replaces CudaRasterizer::Rasterizer::{forward,backward,markVisible}
// (cuda_rasterizer/rasterizer_impl.cu:162-174, 227-411, 416-518).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "gsr_internal.h"
#include "../../include/gsr_aa.h"
#include "../../include/gsr_contrib.h"
#include "../../include/gsr_features.h"
#include "../../include/gsr_distortion.h"
#include "../../include/gsr_median.h"
#include "../../include/gsr_normals.h"
#include "../../include/gsr_loss_ext.h"
#include "../../include/gsr_bilagrid.h"
#include "../../include/gsr_mcmc.h"
#include "../../include/gsr_densify.h"
#include "../../include/gsr_filter3d.h"
#include "../../include/gsr_slice4d.h"
#include "../../include/gsr_tsdf.h"
#include "../../include/gsr_vq.h"
#include "../../include/gsr_knn.h"
#include "../../include/gsr_rigidity.h"

#define GSR_MAX_DEVICES 64
// Beside the depth sort the SH colour kernel is held to two workgroups per CU (unused dynamic LDS on top of its staging area): it has
// until the end of the depth sort to finish, and at full occupancy its memory traffic doubled the latency-bound first launches of
// that sort (histogram 6 -> 15 us, scatter 13 -> 25).  Measured at C3: step 1.167 -> 1.160 ms with two workgroups per CU (three:
// 1.161, one: 1.161).  Only while the colour kernel is the shorter of the two: its time grows with P, the depth sort's barely (C5,
// 6M Gaussians: colour 0.42 ms against 0.25 ms of sort -- there it keeps the whole chip).  (Round 4: the limit used to be a fixed
// 40 KB of dynamic LDS, which on top of the 52 KB the LEAF kernel then staged left ONE workgroup per CU -- 0.224 ms instead of 0.06, and
// the training iteration's binning waited 110 us for it: profiles/r4_train_iteration_timeline_before.txt; the leaf kernel now stages
// in halves like the packed one.)
#ifndef GSR_COLOR_BESIDE_WGS
#define GSR_COLOR_BESIDE_WGS 2
#endif
// (Measured and not kept, round 4: the colour kernel in two pieces -- 40 / 55 / 70 % of its workgroups beside the geometry kernel, the
// rest held back by an event until the bucket depth sort's last kernel had finished, i.e. beside the binning kernels instead of the
// sort's round trips -- step 1.092 -> 1.107-1.110 ms at C3: the held-back piece ends after the binning does and the join waits for it.)
#define GSR_COLOR_BESIDE_MAX_P 1500000

// ---- errors ------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

int gsr_fail(int code, const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof g_err, fmt, ap);
	va_end(ap);
	return code;
}

int gsr_check_hip(hipError_t e, const char* what)
{
	if (e == hipSuccess) return GSR_OK;
	return gsr_fail(GSR_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

int gsr_stage_done(hipStream_t s, int debug, const char* stage)
{
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return gsr_fail(GSR_ERR_HIP, "launch of %s failed: %s", stage, hipGetErrorString(e));
	if (debug & GSR_DEBUG_SYNC) {  // CHECK_CUDA semantics, auxiliary.h:177-184
		e = hipStreamSynchronize(s);
		if (e != hipSuccess) return gsr_fail(GSR_ERR_HIP, "[HIP ERROR] in stage %s: %s", stage, hipGetErrorString(e));
	}
	return GSR_OK;
}

extern "C" const char* gsr_last_error(void) { return g_err; }
extern "C" const char* gsr_version(void) { return "gsr-hip gfx950 r4"; }

// ---- per-kernel event profiling ----------------------------------------------------------------
// One recorder per stream that asked for it (gsr_profile_begin(stream)).  A stage looks its stream up; with no
// recorder active anywhere that is one relaxed atomic load.  Events come from a pool that only grows, so
// recording inside a timed region costs two hipEventRecord per stage and no allocation after the first step.
// Nothing here is keyed by thread: PyTorch runs the backward on its own autograd thread, one per device, and
// each of them is told apart by the stream it passes.
struct ProfEntry { const char* name; hipEvent_t a, b; };
struct ProfRecorder {
	hipStream_t stream;
	bool on = false, open = false;
	std::vector<ProfEntry> ev;
	size_t used = 0;
	char only[64] = "";  // when non-empty: record this stage only (every hipEventRecord drains the queue ~5 us)
};
static std::mutex g_prof_mu;
static std::vector<ProfRecorder*> g_prof;  // guarded by g_prof_mu; recorders are kept for reuse of their events
static std::atomic<int> g_prof_active{0};

static ProfRecorder* prof_find(hipStream_t s, bool create)
{
	for (ProfRecorder* r : g_prof)
		if (r->stream == s) return r;
	if (!create) return nullptr;
	ProfRecorder* r = new ProfRecorder();
	r->stream = s;
	g_prof.push_back(r);
	return r;
}

// the next event pair of the pool, which grows when all are in use
static ProfEntry& prof_next(ProfRecorder* r, const char* name)
{
	if (r->used == r->ev.size()) {
		ProfEntry e;
		e.name = name;
		(void)hipEventCreate(&e.a);
		(void)hipEventCreate(&e.b);
		r->ev.push_back(e);
	}
	ProfEntry& e = r->ev[r->used++];
	e.name = name;
	return e;
}

// Single-stage recording of a stage that is ONE kernel: the events its launcher hands to gsr_launch as start / stop events -- the
// kernel's own dispatch packet takes the two timestamps, no hipEventRecord stands in front of or behind it.  false: not recording
// this stage that way.
bool gsr_prof_kernel_events(hipStream_t s, const char* name, hipEvent_t* a, hipEvent_t* b)
{
	if (g_prof_active.load(std::memory_order_relaxed) == 0) return false;
	std::lock_guard<std::mutex> lk(g_prof_mu);
	ProfRecorder* r = prof_find(s, false);
	if (!r || !r->on || !r->only[0] || strcmp(r->only, name) != 0) return false;
	ProfEntry& e = prof_next(r, name);
	r->open = false;
	*a = e.a;
	*b = e.b;
	return true;
}

void gsr_prof_mark_begin(hipStream_t s, const char* name)
{
	if (!name || g_prof_active.load(std::memory_order_relaxed) == 0) return;
	std::lock_guard<std::mutex> lk(g_prof_mu);
	ProfRecorder* r = prof_find(s, false);
	if (!r || !r->on) return;
	r->open = false;
	if (r->only[0] && strcmp(r->only, name) != 0) return;
	r->open = true;
	(void)hipEventRecord(prof_next(r, name).a, s);
}

void gsr_prof_mark_end(hipStream_t s)
{
	if (g_prof_active.load(std::memory_order_relaxed) == 0) return;
	std::lock_guard<std::mutex> lk(g_prof_mu);
	ProfRecorder* r = prof_find(s, false);
	if (!r || !r->on || !r->open || r->used == 0) return;
	r->open = false;
	(void)hipEventRecord(r->ev[r->used - 1].b, s);
}

// true while a recorder on this stream records EVERY stage (bench.py's per-kernel table): stages that normally
// overlap on a helper stream then run in line, so that each gets a time of its own
static bool gsr_prof_records_all(hipStream_t s)
{
	if (g_prof_active.load(std::memory_order_relaxed) == 0) return false;
	std::lock_guard<std::mutex> lk(g_prof_mu);
	ProfRecorder* r = prof_find(s, false);
	return r && r->on && !r->only[0];
}

extern "C" int gsr_profile_begin_only(void* stream, const char* stage)
{
	std::lock_guard<std::mutex> lk(g_prof_mu);
	ProfRecorder* r = prof_find((hipStream_t)stream, true);
	if (!r->on) g_prof_active.fetch_add(1);
	r->on = true;
	r->open = false;
	r->used = 0;
	r->only[0] = 0;
	if (stage) { strncpy(r->only, stage, sizeof r->only - 1); r->only[sizeof r->only - 1] = 0; }
	return GSR_OK;
}

extern "C" int gsr_profile_begin(void* stream) { return gsr_profile_begin_only(stream, nullptr); }

extern "C" int gsr_profile_end(void* stream, gsr_kernel_time* out, int capacity)
{
	std::lock_guard<std::mutex> lk(g_prof_mu);
	ProfRecorder* r = prof_find((hipStream_t)stream, false);
	if (!r || !r->on) return 0;
	r->on = false;
	g_prof_active.fetch_sub(1);
	int n = 0;
	for (size_t k = 0; k < r->used; k++) {
		ProfEntry& e = r->ev[k];
		(void)hipEventSynchronize(e.b);
		float ms = 0.f;
		(void)hipEventElapsedTime(&ms, e.a, e.b);
		if (out && n < capacity) { out[n].name = e.name; out[n].ms = ms; n++; }
	}
	r->used = 0;
	return n;
}

// ---- layouts -----------------------------------------------------------------------------------
extern "C" int gsr_geometry_layout_of(int P, gsr_geometry_layout* o)
{
	if (P < 0 || !o) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_geometry_layout_of: bad arguments");
	const size_t n = (size_t)P;
	const size_t nb = (n + GSR_PREPROCESS_BLOCK - 1) / GSR_PREPROCESS_BLOCK;
	size_t off = 0;
	o->splat = off;          off = gsr_align_up(off + n * sizeof(GsrSplat));
	o->depth_keys = off;     off = gsr_align_up(off + n * 4);
	o->depth_keys_alt = off; off = gsr_align_up(off + n * 4);
	o->perm = off;           off = gsr_align_up(off + n * 4);
	o->perm_alt = off;       off = gsr_align_up(off + n * 4);
	o->tiles_touched = off;  off = gsr_align_up(off + n * 4);
	o->rect = off;           off = gsr_align_up(off + n * 8);
	o->slot_base = off;      off = gsr_align_up(off + n * 4);
	o->clamped = off;        off = gsr_align_up(off + n);
	o->sh_ddir = off;        off = gsr_align_up(off + n * 36);
	o->status = off;         off = gsr_align_up(off + GSR_STATUS_WORDS * 4);
	o->scan_temp = off;      off = gsr_align_up(off + 2 * gsr_align_up(nb * 4));   // depth-ordered block sums, then the preprocess workgroups' tile counts
	o->sort_table = off;     off = gsr_align_up(off + gsr_radix_table_bytes(n));
	o->col_table = off;      off = gsr_align_up(off + gsr_tilebin_col_table_bytes(n));
	o->rshape = off;         off = gsr_align_up(off + n * 8);
	o->total = off;
	return GSR_OK;
}

extern "C" int gsr_image_layout_of(int W, int H, gsr_image_layout* o)
{
	if (W < 0 || H < 0 || !o) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_image_layout_of: bad arguments");
	const size_t N = (size_t)W * H, T = (size_t)gsr_grid_x(W) * gsr_grid_y(H);
	size_t off = 0;
	o->final_C = off;          off = gsr_align_up(off + 3 * N * 4);
	o->final_T = off;          off = gsr_align_up(off + N * 4);
	o->n_contrib = off;        off = gsr_align_up(off + N * 4);
	o->ranges = off;           off = gsr_align_up(off + T * 8);
	o->tile_max_contrib = off; off = gsr_align_up(off + T * 4);
	{
		const size_t extra_f = 3 * (size_t)gsr_tile_order_max_split((int)T), extra_b = gsr_tile_order_max_segments((int)T);
		o->tile_order = off;   off = gsr_align_up(off + (T + (extra_f > extra_b ? extra_f : extra_b) + 1) * 4);   // + the segment coarseness word
	}
	o->total = off;
	return GSR_OK;
}

extern "C" int gsr_binning_layout_of(int P, int64_t R, int W, int H, gsr_binning_layout* o)
{
	(void)P;
	if (R < 0 || W < 0 || H < 0 || !o) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_binning_layout_of: bad arguments");
	const size_t n = (size_t)R;
	size_t off = 0;
	o->point_list = off;     off = gsr_align_up(off + n * 4);
	o->point_list_alt = off; off = gsr_align_up(off + n * 4);
	o->tile_keys = off;      off = gsr_align_up(off + n * 4);
	// the forward's band masks: R bytes of tile_keys_alt behind the validity bytes (which tile_ranges / row_scatter clear in whole words:
	// hence the rounding).  4 ceil(R / 4) + R <= 4 R from R = 2 on, and the array is never smaller than 256 bytes.
	o->band_masks = off + gsr_align_up(n, 4);
	o->tile_keys_alt = off;  off = gsr_align_up(off + n * 4);
	{
		const size_t a = gsr_radix_table_bytes(n), b = gsr_tilebin_row_table_bytes(n);   // tile sort (sort.hip) / pass 2 of tilebin.hip
		o->sort_table = off; off = gsr_align_up(off + (a > b ? a : b));
	}
	o->checkpoints = off;    off = gsr_align_up(off + gsr_checkpoint_records(R) * 256 * sizeof(float4));
	o->total = off;
	o->tile_key_bytes = (size_t)gsr_tile_key_bytes(gsr_grid_x(W) * gsr_grid_y(H), n);
	o->column_pairs = gsr_tilebin_applies(W, H) ? 1 : 0;
	return GSR_OK;
}

extern "C" size_t gsr_geometry_bytes(int P)
{
	gsr_geometry_layout l;
	return gsr_geometry_layout_of(P, &l) == GSR_OK ? l.total : 0;
}
extern "C" size_t gsr_image_bytes(int W, int H)
{
	gsr_image_layout l;
	return gsr_image_layout_of(W, H, &l) == GSR_OK ? l.total : 0;
}
extern "C" size_t gsr_binning_bytes(int P, int64_t R, int W, int H)
{
	gsr_binning_layout l;
	return gsr_binning_layout_of(P, R, W, H, &l) == GSR_OK ? l.total : 0;
}
extern "C" size_t gsr_backward_scratch_bytes(int P, int64_t R)
{
	(void)P;
	if (R < 0) return 0;
	return gsr_align_up((size_t)R * sizeof(GsrGradSlot));
}

// ---- depth and alpha maps: the scratch the forward leaves for the backward -----------------------
extern "C" int gsr_aux_layout_of(int64_t R, int W, int H, gsr_aux_layout* o)
{
	if (R < 0 || W < 0 || H < 0 || !o) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_aux_layout_of: bad arguments");
	size_t off = 0;
	o->ckpt_depth = off; off = gsr_align_up(off + gsr_checkpoint_records(R) * 256 * sizeof(float));
	o->final_D = off;    off = gsr_align_up(off + (size_t)W * H * sizeof(float));
	o->total = off;
	return GSR_OK;
}
extern "C" size_t gsr_aux_bytes(int64_t R, int W, int H)
{
	gsr_aux_layout l;
	return gsr_aux_layout_of(R, W, H, &l) == GSR_OK ? l.total : 0;
}
// what the blend launchers take: NULL without the maps, else `a` filled from the caller's arguments
static const GsrAuxBlend* gsr_aux_view(const gsr_aux_args* x, int64_t R, int W, int H, GsrAuxBlend* a)
{
	if (!x) return nullptr;
	gsr_aux_layout l;
	gsr_aux_layout_of(R, W, H, &l);
	char* b = (char*)x->scratch;
	a->out_depth = x->out_depth; a->out_alpha = x->out_alpha;
	a->ckpt_depth = (float*)(b + l.ckpt_depth);
	a->final_D = (float*)(b + l.final_D);
	a->dL_ddepth = x->dL_ddepth; a->dL_dalpha = x->dL_dalpha;
	return a;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// The validity check of the option arguments (include/gsr_aux.h, include/gsr_aa.h): called by gsr_gaussian_options for the per-Gaussian
// passes, and by the blend's *_aux / *_abs entry points themselves.  antialiasing: 0 or 1 (the *_aux calls pass 0).  aux: NULL only
// where `optional` (the *_aa calls); its mode is always checked, and beyond that what the calling stage needs of it.  live: the call
// has work to launch, so what it needs must be there.
enum GsrAuxNeeds {
	GSR_AUX_NEEDS_MODE,      // stage 1: reads nothing else
	GSR_AUX_NEEDS_SCRATCH,   // the backward: an aligned scratch (the blend reads it; the per-Gaussian pass takes the same arguments)
	GSR_AUX_NEEDS_OUTPUTS    // the forward blend: the two maps and the scratch
};
static int gsr_option_check(const char* who, int antialiasing, const gsr_aux_args* aux, bool optional, GsrAuxNeeds needs, bool live)
{
	if (antialiasing != 0 && antialiasing != 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: antialiasing must be 0 or 1, got %d", who, antialiasing);
	if (!aux) return optional ? GSR_OK : gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: aux is NULL", who);
	if (aux->mode != GSR_AUX_DEPTH && aux->mode != GSR_AUX_INVDEPTH) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: the mode of aux is unknown", who);
	if (needs == GSR_AUX_NEEDS_MODE) return GSR_OK;
	if (!aligned16(aux->scratch)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: scratch must be 16-byte aligned", who);
	if (live && (!aux->scratch || (needs == GSR_AUX_NEEDS_OUTPUTS && (!aux->out_depth || !aux->out_alpha))))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: %sscratch is NULL", who, needs == GSR_AUX_NEEDS_OUTPUTS ? "out_depth, out_alpha or " : "");
	return GSR_OK;
}

// The validity check of a camera model (include/gsr_camera_model.h), called by gsr_gaussian_options
static int gsr_camera_model_check(const char* who, const gsr_camera_model& m)
{
	if (m.model != GSR_CAMERA_PINHOLE && m.model != GSR_CAMERA_FISHEYE)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: unknown camera model %d", who, m.model);
	if (!(m.fx > 0.f) || !(m.fy > 0.f) || !std::isfinite(m.fx) || !std::isfinite(m.fy))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: fx and fy must be finite and positive, got %g, %g", who, (double)m.fx, (double)m.fy);
	if (!std::isfinite(m.cx) || !std::isfinite(m.cy))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: cx and cy must be finite, got %g, %g", who, (double)m.cx, (double)m.cy);
	return GSR_OK;
}

// ---- the options of the per-Gaussian passes (GsrGaussianOptions) -----------------------------------
// The one check of what the *_aux, *_aa, *_cm, *_cam and *_cam_cm entry points of stage 1 and of the per-Gaussian backward add to the
// plain call, under the caller's name `who`, and the record the pass then runs with.  aux_required: the *_aux calls (elsewhere NULL =
// no maps).  needs: what the stage reads of aux -- GSR_AUX_NEEDS_MODE is stage 1, whose own arguments gsr_forward_preprocess_impl
// checks; else the backward with its args, opacity input and range.  model, cam: NULL = not offered by the caller or not asked for.
static int gsr_gaussian_options(GsrGaussianOptions* o, const char* who, bool aux_required, GsrAuxNeeds needs, const gsr_aux_args* aux,
                                int antialiasing, const float* opacities, const gsr_camera_model* model, const GsrCamTarget* cam,
                                const gsr_backward_args* args, int first, int count)
{
	int rc;
	if (model && (rc = gsr_camera_model_check(who, *model))) return rc;
	if ((rc = gsr_option_check(who, antialiasing, aux, !aux_required, needs, false))) return rc;
	*o = GsrGaussianOptions{};
	o->aux = aux ? aux->mode : 0;
	o->aa = antialiasing;
	o->cm = model;
	if (needs == GSR_AUX_NEEDS_MODE) return GSR_OK;
	if (!args) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: args is NULL", who);
	const gsr_backward_args& a = *args;
	// (under a model the sizes and the geometry buffer are refused under this call's name; without one, by the pass itself)
	if (model && (a.P < 0 || a.num_rendered < 0 || a.width <= 0 || a.height <= 0)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: bad sizes", who);
	if (cam) {
		if (!cam->dL_dviewmatrix || !cam->dL_dmid || !cam->dL_dcampos)
			return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: dL_dviewmatrix, %s or dL_dcampos is NULL", who, model ? "dL_dintrinsics" : "dL_dprojmatrix");
		if (!cam->rows) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: the scratch of cam is NULL", who);
		if (!aligned16(cam->rows)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: the scratch of cam must be 16-byte aligned", who);
		if (first != 0 || count != a.P)
			return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: camera gradients need the whole scene in one call (first 0, count %d; got %d, %d): "
			                "the part-by-part pipeline of view-parallel mode has no camera form", who, a.P, first, count);
		o->cam = *cam;
	}
	if (model && a.P > 0 && !a.geometry) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: geometry is NULL", who);
	if (cam && a.P > 0 && a.shs && !a.cam_pos) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: cam_pos is NULL", who);
	if (antialiasing && a.P > 0 && count > 0 && !opacities) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: the opacity input is NULL", who);
	o->aa_opacities = antialiasing ? opacities : nullptr;
	return GSR_OK;
}

// ---- stages --------------------------------------------------------------------------------------
// One stage of a call: `launch` -- its kernels, and the fills that belong to them -- inside the stage's profiling scope, then
// gsr_stage_done.  launch returns nothing, or a GSR code that ends the call unless it is GSR_OK.  record = false: no scope, because the
// stage is ONE kernel whose own dispatch packet takes the timestamps (gsr_prof_kernel_events).  `launch` is a template parameter, not a
// std::function: the stages are the launch path.
template <typename F>
static int gsr_stage(hipStream_t s, int debug, const char* name, F&& launch, bool record = true)
{
	{
		GsrProfScope p(s, record ? name : nullptr);
		if constexpr (std::is_void<decltype(launch())>::value) launch();
		else if (int rc = launch()) return rc;
	}
	return gsr_stage_done(s, debug, name);
}

// ---- the state of a forward (GsrFrame) -------------------------------------------------------------
// Every call after stage 1 opens the state it reads here, in two steps around its own checks, so that refusals keep one order:
// gsr_frame_sizes (which also clears the last error); the call's option checks; P == 0 is GSR_OK; the call's own pointers;
// gsr_frame_open -- NULL state, alignment, the limit on R; then the call's R == 0 shortcut.
enum : unsigned {
	GSR_FRAME_IMAGE = 1,   // the call reads the image buffer
	GSR_FRAME_SLOTS = 2,   // ... and the gradient slots: like binning, required when R > 0
	GSR_FRAME_R32 = 4      // the call refuses R beyond 32 bits (the blend's and the per-Gaussian backward never have)
};

static int gsr_frame_sizes(const char* who, int P, int64_t R, int W, int H)
{
	g_err[0] = 0;
	if (P < 0 || R < 0 || W <= 0 || H <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: bad sizes", who);
	return GSR_OK;
}

// own_aligned: the call's own buffers that must be 16-byte aligned are (they are refused with the state buffers)
static int gsr_frame_open(GsrFrame* f, const char* who, unsigned needs, int P, int64_t R, int W, int H, const void* geometry, const void* binning,
                          const void* image, void* slots, void* stream, int debug, bool own_aligned)
{
	const bool img = needs & GSR_FRAME_IMAGE, sl = needs & GSR_FRAME_SLOTS;
	if (!geometry || (img && !image) || (R > 0 && (!binning || (sl && !slots))))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: required pointer is NULL", who);
	if (!aligned16(geometry) || (img && !aligned16(image)) || !aligned16(binning) || (sl && !aligned16(slots)) || !own_aligned)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: state buffers and scratch must be 16-byte aligned", who);
	if ((needs & GSR_FRAME_R32) && R > 0xffffffffLL) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: num_rendered exceeds 32-bit offsets", who);
	*f = GsrFrame{};
	f->P = P; f->W = W; f->H = H; f->R = R;
	f->g = gsr_geometry_view((void*)geometry, P);
	if (img) f->img = gsr_image_view((void*)image, W, H);
	if (R > 0) {
		f->bin = gsr_binning_view((void*)binning, P, R, W, H);
		f->slot_valid = (uint8_t*)f->bin.tile_keys_alt;
	}
	if (sl) f->slots = (GsrGradSlot*)slots;
	f->s = (hipStream_t)stream; f->debug = debug; f->cull = !(debug & GSR_DEBUG_NO_CULL);
	return GSR_OK;
}

// the calls that take their state in gsr_backward_args
static int gsr_frame_sizes(const char* who, const gsr_backward_args* a)
{
	g_err[0] = 0;
	if (!a) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: args is NULL", who);
	return gsr_frame_sizes(who, a->P, a->num_rendered, a->width, a->height);
}
static int gsr_frame_open(GsrFrame* f, const char* who, unsigned needs, const gsr_backward_args& a, bool own_aligned)
{
	return gsr_frame_open(f, who, needs, a.P, a.num_rendered, a.width, a.height, a.geometry, a.binning, a.image, a.scratch, a.stream, a.debug, own_aligned);
}

GsrGeometry gsr_geometry_view(void* blob, int P)
{
	gsr_geometry_layout l;
	gsr_geometry_layout_of(P, &l);
	char* b = (char*)blob;
	GsrGeometry g;
	g.splat = (GsrSplat*)(b + l.splat);
	g.depth_keys = (uint32_t*)(b + l.depth_keys);
	g.depth_keys_alt = (uint32_t*)(b + l.depth_keys_alt);
	g.perm = (uint32_t*)(b + l.perm);
	g.perm_alt = (uint32_t*)(b + l.perm_alt);
	g.tiles_touched = (uint32_t*)(b + l.tiles_touched);
	g.rect = (uint2*)(b + l.rect);
	g.slot_base = (uint32_t*)(b + l.slot_base);
	g.clamped = (uint8_t*)(b + l.clamped);
	g.sh_ddir = (float*)(b + l.sh_ddir);
	g.status = (uint32_t*)(b + l.status);
	g.sorted_block_sums = (uint32_t*)(b + l.scan_temp);
	g.block_tiles = (uint32_t*)(b + l.scan_temp + gsr_align_up(((size_t)P + GSR_PREPROCESS_BLOCK - 1) / GSR_PREPROCESS_BLOCK * 4));
	g.sort_table = (void*)(b + l.sort_table);
	g.col_table = (void*)(b + l.col_table);
	g.rshape = (uint2*)(b + l.rshape);
	return g;
}

GsrImage gsr_image_view(void* blob, int W, int H)
{
	gsr_image_layout l;
	gsr_image_layout_of(W, H, &l);
	char* b = (char*)blob;
	GsrImage im;
	im.final_C = (float*)(b + l.final_C);
	im.final_T = (float*)(b + l.final_T);
	im.n_contrib = (uint32_t*)(b + l.n_contrib);
	im.ranges = (uint2*)(b + l.ranges);
	im.tile_max_contrib = (uint32_t*)(b + l.tile_max_contrib);
	im.tile_order = (uint32_t*)(b + l.tile_order);
	return im;
}

GsrBinning gsr_binning_view(void* blob, int P, int64_t R, int W, int H)
{
	gsr_binning_layout l;
	gsr_binning_layout_of(P, R, W, H, &l);
	char* b = (char*)blob;
	GsrBinning bn;
	bn.point_list = (uint32_t*)(b + l.point_list);
	bn.point_list_alt = (uint32_t*)(b + l.point_list_alt);
	bn.tile_keys = (uint32_t*)(b + l.tile_keys);
	bn.tile_keys_alt = (uint32_t*)(b + l.tile_keys_alt);
	bn.band_masks = (uint8_t*)(b + l.band_masks);
	bn.sort_table = (void*)(b + l.sort_table);
	bn.checkpoints = (float4*)(b + l.checkpoints);
	return bn;
}

// rasterizer_impl.cu:37-52
extern "C" uint32_t gsr_get_higher_msb(uint32_t n)
{
	uint32_t msb = sizeof(n) * 4;
	uint32_t step = msb;
	while (step > 1) {
		step /= 2;
		if (n >> msb) msb += step; else msb -= step;
	}
	if (n >> msb) msb++;
	return msb;
}

// ---- per-thread helper resources -----------------------------------------------------------------
// One helper stream (+ fork / join events) and one pinned landing buffer (+ its event) per host thread and device, created
// on first use by gsr_forward_preprocess*.  They are the only things the library keeps between calls; a thread that is
// done with the library returns them with gsr_thread_release().
struct GsrThreadDevice {
	hipStream_t aux_stream = nullptr;
	hipEvent_t aux_fork = nullptr, aux_join = nullptr;
	uint32_t* status_host = nullptr;
	hipEvent_t status_event = nullptr;
	hipStream_t copy_stream = nullptr;   // the count's read-back travels beside the depth sort, not in front of it
	hipEvent_t copy_fork = nullptr;
};
struct GsrThreadState { GsrThreadDevice dev[GSR_MAX_DEVICES]; };
static thread_local GsrThreadState g_thread;

extern "C" int gsr_thread_release(void)
{
	g_err[0] = 0;
	int rc = GSR_OK;
	for (int d = 0; d < GSR_MAX_DEVICES; d++) {
		GsrThreadDevice& t = g_thread.dev[d];
		// the helper stream's work was joined into the caller's stream by every call; draining it here covers a caller
		// that releases while its own stream still runs
		if (t.aux_stream) { (void)hipStreamSynchronize(t.aux_stream); if (hipStreamDestroy(t.aux_stream) != hipSuccess) rc = GSR_ERR_HIP; }
		if (t.aux_fork && hipEventDestroy(t.aux_fork) != hipSuccess) rc = GSR_ERR_HIP;
		if (t.aux_join && hipEventDestroy(t.aux_join) != hipSuccess) rc = GSR_ERR_HIP;
		if (t.status_event && hipEventDestroy(t.status_event) != hipSuccess) rc = GSR_ERR_HIP;
		if (t.copy_stream) { (void)hipStreamSynchronize(t.copy_stream); if (hipStreamDestroy(t.copy_stream) != hipSuccess) rc = GSR_ERR_HIP; }
		if (t.copy_fork && hipEventDestroy(t.copy_fork) != hipSuccess) rc = GSR_ERR_HIP;
		if (t.status_host && hipHostFree(t.status_host) != hipSuccess) rc = GSR_ERR_HIP;
		t = GsrThreadDevice();
	}
	if (rc) { (void)hipGetLastError(); return gsr_fail(rc, "gsr_thread_release: a HIP resource could not be freed"); }
	return GSR_OK;
}

// A helper stream of this thread, created on first use: a non-blocking stream and its events (e1 may be NULL: none).  false: they
// cannot be had, nothing is kept, and the caller runs that work in line.
static bool gsr_helper_stream(hipStream_t* stream, hipEvent_t* e0, hipEvent_t* e1)
{
	if (*stream) return true;
	hipStream_t st = nullptr;
	hipEvent_t a = nullptr, b = nullptr;
	if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&a, hipEventDisableTiming) == hipSuccess &&
	    (!e1 || hipEventCreateWithFlags(&b, hipEventDisableTiming) == hipSuccess)) {
		*stream = st; *e0 = a;
		if (e1) *e1 = b;
		return true;
	}
	(void)hipGetLastError();
	if (st) (void)hipStreamDestroy(st);
	if (a) (void)hipEventDestroy(a);
	if (b) (void)hipEventDestroy(b);
	return false;
}

// Makes `stream` wait for the helper stream's join event when the scope ends, unless now() already did.
struct GsrJoinOnExit {
	hipStream_t s;
	hipEvent_t ev = nullptr;
	explicit GsrJoinOnExit(hipStream_t st) : s(st) {}
	void arm(hipEvent_t e) { ev = e; }
	int now()
	{
		if (!ev) return GSR_OK;
		hipEvent_t e = ev;
		ev = nullptr;
		if (hipStreamWaitEvent(s, e, 0) == hipSuccess) return GSR_OK;
		(void)hipEventSynchronize(e);  // the stream could not be made to wait: the host waits instead
		return gsr_fail(GSR_ERR_HIP, "hipStreamWaitEvent(join) failed");
	}
	~GsrJoinOnExit()
	{
		if (ev && hipStreamWaitEvent(s, ev, 0) != hipSuccess) (void)hipEventSynchronize(ev);
	}
};

// Drains the count's read-back stream when the scope ends, unless the host has already waited for the copy: the blit reads
// geometry->status, and include/gsr.h promises that nothing of it outlives the call -- on the error returns too.
struct GsrDrainOnExit {
	hipStream_t st = nullptr;
	void arm(hipStream_t s) { st = s; }
	void disarm() { st = nullptr; }
	~GsrDrainOnExit() { if (st) (void)hipStreamSynchronize(st); }
};

// What stage 1 last chose on this host thread (binning by column pairs or by the tile sort), and for which geometry buffer: stage 2
// re-derives the choice from its own `debug` argument, and a caller that passes GSR_DEBUG_TILE_SORT to one call only would otherwise
// get a point_list built from tables that were never filled.
struct GsrLastStage1 { const void* geometry = nullptr; bool col_pairs = false; };
static thread_local GsrLastStage1 g_last_stage1;

// ---- forward, stage 1 --------------------------------------------------------------------------
// `in`: the caller's inputs (gsr_preprocess_inputs / gsr_preprocess_leaves); what stage 1 derives itself (focal lengths, trim, the
// geometry view) is filled in here.  o: the checked options, which stay outside the struct (it is the kernels' argument); under a
// camera model projmatrix and the tangents are not read.
static int gsr_forward_preprocess_impl(const GsrPreprocessArgs& in, void* geometry, int64_t* num_rendered_host, void* stream, int debug,
                                       const GsrGaussianOptions& o)
{
	g_err[0] = 0;
	hipStream_t s = (hipStream_t)stream;
	GsrPreprocessArgs a = in;
	const int P = a.P, width = a.W, height = a.H;
	if (!num_rendered_host) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "num_rendered_host is NULL");
	*num_rendered_host = 0;
	if (P < 0 || width <= 0 || height <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "bad P / image size");
	if (P == 0) return GSR_OK;  // rasterize_points.cu:94: nothing is launched for an empty scene
	if (!a.means3D || !a.opacities || !a.viewmatrix || (!a.projmatrix && !o.cm) || !geometry)  // radii is optional (rasterizer.h:52)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_forward_preprocess: required pointer is NULL");
	if (!a.colors_precomp && !a.shs)  // rasterizer_impl.cu:281-284
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "For non-RGB, provide precomputed Gaussian colors!");
	if (!a.colors_precomp && (a.M <= 0 || (a.D + 1) * (a.D + 1) > a.M || a.D < 0 || a.D > 3 || !a.cam_pos))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "SH degree %d needs %d coefficients, M = %d", a.D, (a.D + 1) * (a.D + 1), a.M);
	if (!a.cov3D_precomp && (!a.scales || !a.rotations))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "provide scales+rotations or cov3D_precomp");
	if (width > 65535 * GSR_TILE_X || height > 65535 * GSR_TILE_Y)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image too large for 16-bit tile coordinates");
	if (!aligned16(geometry)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "geometry buffer must be 16-byte aligned");

	if (a.leaf && (a.M > 1 && !a.shs_rest)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "leaf mode: features_rest is NULL");
	if (a.leaf && a.M > 16) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "leaf mode: at most 16 SH coefficients (degree 3), M = %d", a.M);
	a.focal_y = height / (2.0f * a.tan_fovy);  // rasterizer_impl.cu:251-252
	a.focal_x = width / (2.0f * a.tan_fovx);
	if (o.cm) { a.focal_x = o.cm->fx; a.focal_y = o.cm->fy; }
	a.g = gsr_geometry_view(geometry, P);

	int rc;
	int device = 0;
	if ((rc = gsr_check_hip(hipGetDevice(&device), "hipGetDevice"))) return rc;
	if (device < 0 || device >= GSR_MAX_DEVICES) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "device index %d not supported", device);
	// The SH colours are needed by nothing before the blend: their kernel runs on a helper stream (one per host thread and
	// device, created on first use, freed by gsr_thread_release()) beside the geometry kernel and the depth sort, whose
	// launches are short and leave most of the chip idle, and is joined before this call's last kernel.  In line instead
	// when every stage is being timed, with GSR_DEBUG_SYNC (a device sync follows every stage) and with GSR_DEBUG_SERIAL.
	GsrThreadDevice& td = g_thread.dev[device];
	const bool col_pairs = gsr_tilebin_applies(width, height) && !(debug & GSR_DEBUG_TILE_SORT);   // (stage 2 decides the same way)
	a.trim = (col_pairs && !(debug & GSR_DEBUG_NO_TRIM)) ? 1 : 0;   // tiles a splat provably misses are left out of the column-pair binning (gsr_rect_trim.h); the tile sort bins them all
	const bool color = gsr_preprocess_needs_color(a);
	// Depth order: up to GSR_BUCKET_SORT_MAX_P Gaussians in three launches whatever the depth range (depthsort.hip: top-digit buckets,
	// then every bucket sorted inside LDS; the result lands in (depth_keys, perm) and the rectangles in depth order come with it).
	// Beyond, and with GSR_DEBUG_RADIX_DEPTH: the global LSD passes.
#ifdef GSR_AB_FORCE_RADIX_DEPTH   // (A/B builds: csrc/Makefile `variant`)
	const bool bucket = false;
#else
	const bool bucket = gsr_bucket_sort_applies(P) && !(debug & GSR_DEBUG_RADIX_DEPTH);
#endif
	// (Measured and not kept, round 3: a lowest-priority helper stream changes nothing -- the depth sort's first histogram
	// and scatter still take 15 + 25 us beside the colour kernel instead of 6 + 13 alone; a helper stream confined to every
	// other CU with hipExtStreamCreateWithCUMask made the step 0.16 ms slower.)
	const bool beside = color && !(debug & (GSR_DEBUG_SYNC | GSR_DEBUG_SERIAL)) && !gsr_prof_records_all(s) &&
	                    gsr_helper_stream(&td.aux_stream, &td.aux_fork, &td.aux_join);   // no helper stream: the colour kernel runs in line
	// From the fork on, EVERY return -- the error returns too -- first makes the caller's stream wait for the colour kernel:
	// the caller is free to release or reuse `geometry` on `stream` the moment this call returns (include/gsr.h, stream
	// contract), and the helper stream may still be writing rgb / clamp bits / sh_ddir into it.
	GsrJoinOnExit join(s);
	// The status words start at zero (a one-workgroup kernel); its dispatch packet signals the helper stream's fork event, so the
	// helper stream starts where the caller's stream stands now (its inputs are ready there) without a barrier packet of its own
	gsr_launch_zero_status(a.g.status, s, beside ? td.aux_fork : nullptr);
	if (beside) {
		if ((rc = gsr_check_hip(hipStreamWaitEvent(td.aux_stream, td.aux_fork, 0), "hipStreamWaitEvent(fork)"))) return rc;
		gsr_launch_preprocess_color(a, td.aux_stream, P <= GSR_COLOR_BESIDE_MAX_P ? GSR_COLOR_BESIDE_WGS : 0, o.aux);
		if (hipEventRecord(td.aux_join, td.aux_stream) != hipSuccess) {
			(void)hipStreamSynchronize(td.aux_stream);  // no event to wait for: wait on the host instead, then report
			return gsr_fail(GSR_ERR_HIP, "hipEventRecord(join) failed");
		}
		join.arm(td.aux_join);
	}
	// The count's read-back (a 6 us blit) goes to a stream of its own behind the geometry kernel, so that the depth sort's first
	// launch follows that kernel directly; the stream waits for an event that the geometry kernel's own dispatch packet signals
	// (gsr_launch) -- a hipEventRecord behind the kernel is a barrier packet and cost the sort's first launch ~8 us.
	// The host waits for the copy before this call returns, so nothing of it outlives the call.  In line with GSR_DEBUG_SYNC /
	// GSR_DEBUG_SERIAL, when every stage is being timed, or when the stream cannot be had.
	const bool copy_beside = !(debug & (GSR_DEBUG_SYNC | GSR_DEBUG_SERIAL)) && !gsr_prof_records_all(s) &&
	                         gsr_helper_stream(&td.copy_stream, &td.copy_fork, nullptr);
	if ((rc = gsr_stage(s, debug, "preprocess", [&] { gsr_launch_preprocess(a, s, copy_beside ? td.copy_fork : nullptr, o); }))) return rc;
	if (color && !beside && (rc = gsr_stage(s, debug, "preprocess_color", [&] { gsr_launch_preprocess_color(a, s, 0, o.aux); }))) return rc;

	// read num_rendered back; the per-Gaussian half of the sort is enqueued behind the copy and keeps
	// the GPU busy while the host waits on the event, allocates the binning buffer and launches stage 2
	// pinned landing buffer + event, created once per (thread, device) and reused
	if (!td.status_host) {
		if ((rc = gsr_check_hip(hipHostMalloc((void**)&td.status_host, GSR_STATUS_WORDS * 4, hipHostMallocDefault), "hipHostMalloc"))) return rc;
	}
	if (!td.status_event) {
		if ((rc = gsr_check_hip(hipEventCreateWithFlags(&td.status_event, hipEventDisableTiming), "hipEventCreate"))) return rc;
	}
	uint32_t* status_host = td.status_host;
	hipEvent_t ev = td.status_event;
	if (copy_beside && (rc = gsr_check_hip(hipStreamWaitEvent(td.copy_stream, td.copy_fork, 0), "hipStreamWaitEvent(copy fork)"))) return rc;
	hipStream_t cs = copy_beside ? td.copy_stream : s;
	GsrDrainOnExit drain;   // from here to the host's wait below every return drains the copy's stream: the copy must not outlive the call
	if (copy_beside) drain.arm(td.copy_stream);
	if ((rc = gsr_check_hip(hipMemcpyAsync(status_host, a.g.status, GSR_STATUS_WORDS * 4, hipMemcpyDeviceToHost, cs), "hipMemcpyAsync(num_rendered)"))) return rc;
	if ((rc = gsr_check_hip(hipEventRecord(ev, cs), "hipEventRecord"))) return rc;
	// The depth sort orders key - min (keys = float bits of the view-space depth; min / max: partial maxima in the status
	// words, reduced by every sort workgroup).  Its first three 8-bit passes are always needed and are enqueued at once;
	// whether bits 24..31 of max - min are populated is known once the status block has landed on the host.
	const uint32_t* bias = a.g.status + GSR_STATUS_NEGMIN;
	rc = gsr_stage(s, debug, "depth_sort", [&] {
		if (bucket) {
			gsr_launch_depth_bucket_sort(a.g, P, col_pairs ? gsr_tilebin_seg(a.g, P) : nullptr, s);
			if (col_pairs) gsr_launch_tilebin_col_hist(a.g, P, 0, s, true);
			else gsr_launch_sorted_block_sums(a.g, P, 0, s);
		} else {
			gsr_radix_sort_passes(a.g.depth_keys, a.g.perm, a.g.depth_keys_alt, a.g.perm_alt, (size_t)P, 32, 4, 0, 3, a.g.sort_table, bias, 4, s);
			// ... and so are the block sums over the three-pass result (the common case) -- with them, for images the column-pair
			// binning handles, the histogram of its first pass (tilebin.hip): the stream then holds work until the host, back from
			// the wait below, has launched stage 2.  A fourth pass redoes them.
			if (col_pairs) gsr_launch_tilebin_col_hist(a.g, P, 1, s);
			else gsr_launch_sorted_block_sums(a.g, P, 1, s);
			// The gradient slots are numbered in index order here too (the bucket sort's first kernel does it on the way): a kernel of its
			// own, and LAST in stage 1 -- nothing reads slot_base before the backward, and in front of the passes it ran beside the colour
			// kernel, which streams the SH rows: 48 MB took 0.10-0.125 ms there at 6 M Gaussians, 0.025 alone.
			gsr_launch_slot_base_finish(a.g.slot_base, a.g.block_tiles, a.g.status, (size_t)P, s);
		}
	});
	if (rc) return rc;
	if ((rc = gsr_check_hip(hipEventSynchronize(ev), "hipEventSynchronize(num_rendered)"))) return rc;
	drain.disarm();   // (the copy has landed)
	g_last_stage1.geometry = geometry;
	g_last_stage1.col_pairs = col_pairs;
	if (status_host[0] & 1u)  // (the join guard makes `stream` wait for the colour kernel first)
		return gsr_fail(GSR_ERR_PREFILTERED, "Point is filtered although prefiltered is set. This shouldn't happen!");
	int64_t total = 0;
	uint32_t negmin = 0, kmax = 0;
	for (int k = 0; k < GSR_COUNT_PARTS; k++) {
		total += (int64_t)status_host[4 + k];
		negmin = status_host[GSR_STATUS_NEGMIN + k] > negmin ? status_host[GSR_STATUS_NEGMIN + k] : negmin;
		kmax = status_host[GSR_STATUS_MAX + k] > kmax ? status_host[GSR_STATUS_MAX + k] : kmax;
	}
	*num_rendered_host = total;
	const uint32_t kmin = ~negmin;
	const uint32_t culled_value = kmax >= kmin ? (kmax - kmin) + 1u : 0u;   // largest biased key (what culled Gaussians sort as)
	const int fourth = !bucket && ((culled_value >> 24) != 0u || (kmax >= kmin && kmax - kmin == 0xFFFFFFFFu));
	// join: everything the caller enqueues after this call comes after the colour kernel too
	if ((rc = join.now())) return rc;
	if (!fourth) return gsr_stage_done(s, debug, "depth_sort");
	return gsr_stage(s, debug, "depth_sort", [&] {
		gsr_radix_sort_passes(a.g.depth_keys, a.g.perm, a.g.depth_keys_alt, a.g.perm_alt, (size_t)P, 32, 4, 3, 1, a.g.sort_table, bias, 4, s);
		// three passes leave the order in (depth_keys_alt, perm_alt), four in (depth_keys, perm): recorded in status[2]
		if (col_pairs) {   // the histogram's chunk sums were added to by the run over the three-pass order
			if (int e = gsr_check_hip(hipMemsetAsync(a.g.col_table, 0, gsr_tilebin_col_clear_words((size_t)P) * 4, s), "hipMemsetAsync(col_table)")) return e;
			gsr_launch_tilebin_col_hist(a.g, P, 0, s);
		} else {
			gsr_launch_sorted_block_sums(a.g, P, 0, s);   // (their prefix sums are taken by the key emission itself)
		}
		return (int)GSR_OK;
	});
}

// the inputs of the calls that take activated tensors, and of the calls that take the optimiser's leaves (activated inside the kernels)
static GsrPreprocessArgs gsr_preprocess_inputs(int P, int D, int M, int width, int height, const float* means3D, const float* shs,
                                               const float* colors_precomp, const float* opacities, const float* scales,
                                               float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                               const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                                               float tan_fovy, int prefiltered, int* radii)
{
	GsrPreprocessArgs a = {};
	a.P = P; a.D = D; a.M = M; a.W = width; a.H = height;
	a.means3D = means3D; a.shs = shs; a.colors_precomp = colors_precomp; a.opacities = opacities;
	a.scales = scales; a.scale_modifier = scale_modifier; a.rotations = rotations; a.cov3D_precomp = cov3D_precomp;
	a.viewmatrix = viewmatrix; a.projmatrix = projmatrix; a.cam_pos = cam_pos;
	a.tan_fovx = tan_fovx; a.tan_fovy = tan_fovy;
	a.prefiltered = prefiltered;
	a.radii = radii;
	return a;
}
static GsrPreprocessArgs gsr_preprocess_leaves(int P, int D, int M, int width, int height, const float* xyz, const float* features_dc,
                                               const float* features_rest, const float* opacity_logits, const float* log_scales,
                                               float scale_modifier, const float* raw_rotations, const float* viewmatrix,
                                               const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                                               int prefiltered, int* radii)
{
	GsrPreprocessArgs a = gsr_preprocess_inputs(P, D, M, width, height, xyz, features_dc, nullptr, opacity_logits, log_scales, scale_modifier,
	                                            raw_rotations, nullptr, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, radii);
	a.leaf = 1; a.shs_rest = features_rest;
	return a;
}

// Every stage-1 entry point: the one check of its options under its own name, then the stage.  Under a model the sizes and the geometry
// buffer are refused under that name as well.
static int gsr_forward_preprocess_opt(const char* who, bool aux_required, const gsr_camera_model* model, int antialiasing, const gsr_aux_args* aux,
                                      const GsrPreprocessArgs& a, void* geometry, int64_t* num_rendered_host, void* stream, int debug)
{
	GsrGaussianOptions o;
	int rc;
	if ((rc = gsr_gaussian_options(&o, who, aux_required, GSR_AUX_NEEDS_MODE, aux, antialiasing, nullptr, model, nullptr, nullptr, 0, 0))) return rc;
	if (model && (a.P < 0 || a.W <= 0 || a.H <= 0)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: bad P / image size", who);
	if (model && a.P > 0 && !geometry) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: geometry is NULL", who);
	return gsr_forward_preprocess_impl(a, geometry, num_rendered_host, stream, debug, o);
}

extern "C" int gsr_forward_preprocess(int P, int D, int M, int width, int height, const float* means3D,
                                      const float* shs, const float* colors_precomp, const float* opacities,
                                      const float* scales, float scale_modifier, const float* rotations,
                                      const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                                      const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered,
                                      int* radii, void* geometry, int64_t* num_rendered_host, void* stream, int debug)
{
	const GsrPreprocessArgs a = gsr_preprocess_inputs(P, D, M, width, height, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations,
	                                                    cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, radii);
	return gsr_forward_preprocess_impl(a, geometry, num_rendered_host, stream, debug, GsrGaussianOptions{});
}

extern "C" int gsr_forward_preprocess_leaf(int P, int D, int M, int width, int height, const float* xyz,
                                           const float* features_dc, const float* features_rest,
                                           const float* opacity_logits, const float* log_scales, float scale_modifier,
                                           const float* raw_rotations, const float* viewmatrix, const float* projmatrix,
                                           const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered,
                                           int* radii, void* geometry, int64_t* num_rendered_host, void* stream,
                                           int debug)
{
	const GsrPreprocessArgs a = gsr_preprocess_leaves(P, D, M, width, height, xyz, features_dc, features_rest, opacity_logits, log_scales, scale_modifier,
	                                                    raw_rotations, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, radii);
	return gsr_forward_preprocess_impl(a, geometry, num_rendered_host, stream, debug, GsrGaussianOptions{});
}

extern "C" int gsr_forward_preprocess_aux(const gsr_aux_args* aux, int P, int D, int M, int width, int height, const float* means3D,
                                          const float* shs, const float* colors_precomp, const float* opacities,
                                          const float* scales, float scale_modifier, const float* rotations,
                                          const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                                          const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered,
                                          int* radii, void* geometry, int64_t* num_rendered_host, void* stream, int debug)
{
	const GsrPreprocessArgs a = gsr_preprocess_inputs(P, D, M, width, height, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations,
	                                                    cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, radii);
	return gsr_forward_preprocess_opt("gsr_forward_preprocess_aux", true, nullptr, 0, aux, a, geometry, num_rendered_host, stream, debug);
}

extern "C" int gsr_forward_preprocess_leaf_aux(const gsr_aux_args* aux, int P, int D, int M, int width, int height, const float* xyz,
                                               const float* features_dc, const float* features_rest,
                                               const float* opacity_logits, const float* log_scales, float scale_modifier,
                                               const float* raw_rotations, const float* viewmatrix, const float* projmatrix,
                                               const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered,
                                               int* radii, void* geometry, int64_t* num_rendered_host, void* stream,
                                               int debug)
{
	const GsrPreprocessArgs a = gsr_preprocess_leaves(P, D, M, width, height, xyz, features_dc, features_rest, opacity_logits, log_scales, scale_modifier,
	                                                    raw_rotations, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, radii);
	return gsr_forward_preprocess_opt("gsr_forward_preprocess_leaf_aux", true, nullptr, 0, aux, a, geometry, num_rendered_host, stream, debug);
}

// the anti-aliased path (include/gsr_aa.h): aux NULL or a known mode; antialiasing 0 or 1
extern "C" int gsr_forward_preprocess_aa(int antialiasing, const gsr_aux_args* aux, int P, int D, int M, int width, int height,
                                         const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                                         const float* scales, float scale_modifier, const float* rotations,
                                         const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                                         const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered,
                                         int* radii, void* geometry, int64_t* num_rendered_host, void* stream, int debug)
{
	const GsrPreprocessArgs a = gsr_preprocess_inputs(P, D, M, width, height, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations,
	                                                    cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, radii);
	return gsr_forward_preprocess_opt("gsr_forward_preprocess_aa", false, nullptr, antialiasing, aux, a, geometry, num_rendered_host, stream, debug);
}

extern "C" int gsr_forward_preprocess_leaf_aa(int antialiasing, const gsr_aux_args* aux, int P, int D, int M, int width, int height,
                                              const float* xyz, const float* features_dc, const float* features_rest,
                                              const float* opacity_logits, const float* log_scales, float scale_modifier,
                                              const float* raw_rotations, const float* viewmatrix, const float* projmatrix,
                                              const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered,
                                              int* radii, void* geometry, int64_t* num_rendered_host, void* stream,
                                              int debug)
{
	const GsrPreprocessArgs a = gsr_preprocess_leaves(P, D, M, width, height, xyz, features_dc, features_rest, opacity_logits, log_scales, scale_modifier,
	                                                    raw_rotations, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, radii);
	return gsr_forward_preprocess_opt("gsr_forward_preprocess_leaf_aa", false, nullptr, antialiasing, aux, a, geometry, num_rendered_host, stream, debug);
}

// a camera model (include/gsr_camera_model.h): model NULL = the *_aa call
extern "C" int gsr_forward_preprocess_cm(const gsr_camera_model* model, int antialiasing, const gsr_aux_args* aux, int P, int D, int M,
                                         int width, int height, const float* means3D, const float* shs, const float* colors_precomp,
                                         const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                                         const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                                         const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, int* radii,
                                         void* geometry, int64_t* num_rendered_host, void* stream, int debug)
{
	const GsrPreprocessArgs a = gsr_preprocess_inputs(P, D, M, width, height, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations,
	                                                    cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, radii);
	return gsr_forward_preprocess_opt(model ? "gsr_forward_preprocess_cm" : "gsr_forward_preprocess_aa", false, model, antialiasing, aux, a, geometry,
	                                  num_rendered_host, stream, debug);
}

extern "C" int gsr_forward_preprocess_leaf_cm(const gsr_camera_model* model, int antialiasing, const gsr_aux_args* aux, int P, int D, int M,
                                              int width, int height, const float* xyz, const float* features_dc,
                                              const float* features_rest, const float* opacity_logits, const float* log_scales,
                                              float scale_modifier, const float* raw_rotations, const float* viewmatrix,
                                              const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                                              int prefiltered, int* radii, void* geometry, int64_t* num_rendered_host, void* stream,
                                              int debug)
{
	const GsrPreprocessArgs a = gsr_preprocess_leaves(P, D, M, width, height, xyz, features_dc, features_rest, opacity_logits, log_scales, scale_modifier,
	                                                    raw_rotations, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, radii);
	return gsr_forward_preprocess_opt(model ? "gsr_forward_preprocess_leaf_cm" : "gsr_forward_preprocess_leaf_aa", false, model, antialiasing, aux, a,
	                                  geometry, num_rendered_host, stream, debug);
}

// ---- forward, stage 2 --------------------------------------------------------------------------
static int gsr_forward_render_impl(int P, int64_t R, int width, int height, const float* background, void* geometry, void* binning, void* image,
                                   float* out_color, void* stream, int debug, const gsr_aux_args* aux)
{
	const char* who = "gsr_forward_render";
	int rc;
	if ((rc = gsr_frame_sizes(who, P, R, width, height))) return rc;
	if (P == 0) return GSR_OK;  // image stays as allocated by the caller (zero-filled in the reference)
	if (!background || !out_color) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: required pointer is NULL", who);
	GsrFrame f;
	if ((rc = gsr_frame_open(&f, who, GSR_FRAME_IMAGE | GSR_FRAME_R32, P, R, width, height, geometry, binning, image, nullptr, stream, debug, true))) return rc;
	if ((int64_t)gsr_grid_x(width) * gsr_grid_y(height) >= (1 << 28))  // dispatch-list entries keep the tile id in 28 bits
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image too large: more than 2^28 tiles");

	const GsrGeometry& g = f.g;
	const GsrBinning& b = f.bin;
	hipStream_t s = f.s;
	const int ntiles = gsr_grid_x(width) * gsr_grid_y(height);
	int key_bytes = 4;
	const bool col_pairs = gsr_tilebin_applies(width, height) && !(debug & GSR_DEBUG_TILE_SORT);   // (as stage 1 decided)
	if (g_last_stage1.geometry == geometry && g_last_stage1.col_pairs != col_pairs)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_forward_render: GSR_DEBUG_TILE_SORT must be passed to both forward calls or to neither "
		                "(gsr_forward_preprocess on this thread prepared this geometry buffer for the other binning)");
	if (R > 0 && col_pairs) {
		// column pairs by tile column, their instances by tile row (tilebin.hip): point_list, ranges and the cleared validity
		// bytes come out of the second pass; no per-instance key is ever stored
		if ((rc = gsr_stage(s, debug, "col_scatter", [&] { gsr_launch_tilebin_col_scatter(g, P, b, R, s); }))) return rc;
		if ((rc = gsr_stage(s, debug, "row_hist", [&] { gsr_launch_tilebin_row_hist(g, P, b, R, s); }))) return rc;
		if ((rc = gsr_stage(s, debug, "row_scatter", [&] { gsr_launch_tilebin_row_scatter(g, P, b, R, f.img.ranges, width, height, s); }))) return rc;
	} else {
		if (R > 0) {
			const int bit = (int)gsr_get_higher_msb((uint32_t)ntiles);  // key bits above the depth word, rasterizer_impl.cu:355
			// emit into whichever buffer pair makes the ping-pong sort finish in (tile_keys, point_list)
			const bool even = gsr_radix_num_passes(bit) % 2 == 0;
			uint32_t *k0 = even ? b.tile_keys : b.tile_keys_alt, *v0 = even ? b.point_list : b.point_list_alt;
			uint32_t *k1 = even ? b.tile_keys_alt : b.tile_keys, *v1 = even ? b.point_list_alt : b.point_list;
			key_bytes = gsr_tile_key_bytes(ntiles, (size_t)R);  // 16-bit tile ids whenever they fit: a quarter less traffic in emission, sort, ranges
			rc = gsr_stage(s, debug, "duplicate_keys", [&] {
				gsr_launch_duplicate_keys(g, P, width, k0, key_bytes, v0, (uint32_t*)b.sort_table, gsr_radix_clear_words((size_t)R), s);
			});
			if (rc) return rc;
			rc = gsr_stage(s, debug, "sort", [&] {
				int in_first = 1;
				gsr_radix_sort_u32(k0, v0, k1, v1, (size_t)R, bit, b.sort_table, &in_first, 0, key_bytes, s);  // chunk sums zeroed by duplicate_keys
			});
			if (rc) return rc;
		}
		if ((rc = gsr_stage(s, debug, "tile_ranges", [&] { gsr_launch_tile_ranges(b.tile_keys, key_bytes, R, f.img.ranges, ntiles, b.tile_keys_alt, s); })))
			return rc;
	}
	// (measured at C3: the forward's own order is worth 33 us of blend time for ~12 us of this kernel and its launch)
	if (R > 0 && (rc = gsr_stage(s, debug, "tile_order", [&] { gsr_launch_tile_order(f.img, ntiles, false, R, !(debug & GSR_DEBUG_NO_SPLIT), s, col_pairs); })))
		return rc;
	return gsr_stage(s, debug, "render_forward", [&] {
		GsrAuxBlend x;
		gsr_launch_render_forward(f, background, out_color, R > 0, gsr_aux_view(aux, R, width, height, &x));
	});
}

extern "C" int gsr_forward_render(int P, int64_t R, int width, int height, const float* background,
                                  const int* radii, void* geometry, void* binning, void* image, float* out_color,
                                  void* stream, int debug)
{
	return gsr_forward_render_impl(P, R, width, height, background, geometry, binning, image, out_color, stream, debug, nullptr);
}

extern "C" int gsr_forward_render_aux(const gsr_aux_args* aux, int P, int64_t R, int width, int height, const float* background,
                                      const int* radii, void* geometry, void* binning, void* image, float* out_color,
                                      void* stream, int debug)
{
	int rc;
	if ((rc = gsr_option_check("gsr_forward_render_aux", 0, aux, false, GSR_AUX_NEEDS_OUTPUTS, P > 0))) return rc;
	return gsr_forward_render_impl(P, R, width, height, background, geometry, binning, image, out_color, stream, debug, aux);
}

// ---- backward ----------------------------------------------------------------------------------
// The checks that the two stages of the backward make of their gsr_backward_args, then the frame.  P == 0: GSR_OK, *f is not opened.
// has_model: a camera model stands in for projmatrix (include/gsr_camera_model.h)
static int gsr_backward_open(GsrFrame* f, const gsr_backward_args* args, const char* who, bool has_model)
{
	int rc;
	if ((rc = gsr_frame_sizes(who, args))) return rc;
	const gsr_backward_args& a = *args;
	if (a.P == 0) return GSR_OK;
	if (!a.background || !a.means3D || !a.viewmatrix || (!a.projmatrix && !has_model) || !a.dL_dpix || !a.dL_dmean2D || !a.dL_dopacity ||
	    !a.dL_dmean3D || !a.dL_dscale || !a.dL_drot)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: required pointer is NULL", who);
	// dL_dconic is an intermediate; dL_dcolor / dL_dcov3D are only results when the colours / covariances were
	// inputs (or, dL_dcolor, in view-parallel mode): NULL = not written
	if (!a.leaf && ((a.colors_precomp && !a.dL_dcolor) || (a.cov3D_precomp && !a.dL_dcov3D) || (a.shs && !a.dL_dsh && !a.dL_dcolor)))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward: the gradient of a provided input is NULL");
	if (a.leaf) {
		if (!a.shs || !a.scales || !a.rotations || (a.M > 1 && !a.shs_rest))
			return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward_leaf: a leaf tensor is NULL");
		if (a.M > 16) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward_leaf: at most 16 SH coefficients (degree 3), M = %d", a.M);
		if ((a.dL_dsh == nullptr) != (a.dL_dsh_rest == nullptr) && a.M > 1)
			return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward_leaf: pass both feature gradients or neither");
		if (!a.dL_dsh && !a.dL_dcolor)
			return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward_leaf: without feature gradients dL_dRGB is required");
	}
	if (a.stat_max_radii2D && !a.radii)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward: stat_max_radii2D needs radii");
	return gsr_frame_open(f, who, GSR_FRAME_IMAGE | GSR_FRAME_SLOTS, a, true);   // (the backward has never limited R)
}

// absgrad: the ABS variant of the blend kernel (include/gsr_absgrad.h)
static int gsr_backward_blend_impl(const gsr_backward_args* args, const gsr_aux_args* aux, bool absgrad)
{
	GsrFrame f;
	int rc;
	if ((rc = gsr_backward_open(&f, args, "gsr_backward_blend", false))) return rc;
	if (args->P == 0 || args->num_rendered == 0) return GSR_OK;
	rc = gsr_stage(f.s, f.debug, "tile_order", [&] {
		gsr_launch_tile_order(f.img, gsr_grid_x(f.W) * gsr_grid_y(f.H), true, f.R, !(f.debug & GSR_DEBUG_NO_SPLIT), f.s);
	});
	if (rc) return rc;
	// (recorded alone -- bench.py's timed region -- the kernel's dispatch packet takes the timestamps itself)
	hipEvent_t t0 = nullptr, t1 = nullptr;
	const bool own = gsr_prof_kernel_events(f.s, "render_backward", &t0, &t1);
	return gsr_stage(f.s, f.debug, "render_backward", [&] {
		GsrAuxBlend x;
		gsr_launch_render_backward(f, args->background, args->dL_dpix, t0, t1, gsr_aux_view(aux, f.R, f.W, f.H, &x), absgrad);
	}, !own);
}

extern "C" int gsr_backward_blend(const gsr_backward_args* args) { return gsr_backward_blend_impl(args, nullptr, false); }

extern "C" int gsr_backward_blend_aux(const gsr_backward_args* args, const gsr_aux_args* aux)
{
	int rc;
	if ((rc = gsr_option_check("gsr_backward_blend_aux", 0, aux, false, GSR_AUX_NEEDS_SCRATCH, args && args->P > 0 && args->num_rendered > 0))) return rc;
	return gsr_backward_blend_impl(args, aux, false);
}

// o.cam.rows: the twin kernels that also store the camera rows, then the fold of those rows
static int gsr_backward_gaussians_impl(const gsr_backward_args* args, int first, int count, int out_row0, const GsrGaussianOptions& o)
{
	GsrFrame f;
	int rc;
	if ((rc = gsr_backward_open(&f, args, "gsr_backward_gaussians", o.cm != nullptr))) return rc;
	const gsr_backward_args& b = *args;
	if (first < 0 || count < 0 || (int64_t)first + count > b.P || (first & 63) || (out_row0 != 0 && out_row0 != first))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward_gaussians: bad range [%d, %d + %d) of %d Gaussians (first must be a multiple "
		                "of 64, out_row0 must be 0 or first)", first, first, count, b.P);
	hipStream_t s = (hipStream_t)b.stream;
	auto fold = [&](int nrows) {   // the rows of the per-Gaussian pass into the outputs, structural zeros included
		return gsr_stage(s, b.debug, "camera_grad", [&] {
			if (o.cm) gsr_launch_cam_cm_fold(o.cam.rows, nrows, o.cam.dL_dviewmatrix, o.cam.dL_dmid, o.cam.dL_dcampos, s);
			else gsr_launch_camera_grad_fold(o.cam.rows, nrows, o.cam.dL_dviewmatrix, o.cam.dL_dmid, o.cam.dL_dcampos, s);
		});
	};
	if (o.cam.rows && count == 0) return fold(0);   // no Gaussian: the fold of no rows writes the zeros
	if (count == 0) return GSR_OK;
	GsrGaussianBackwardArgs a = {};
	a.leaf = b.leaf; a.shs_rest = b.shs_rest; a.dL_dsh_rest = b.dL_dsh_rest;
	a.P = b.P; a.D = b.D; a.M = b.M; a.W = b.width; a.H = b.height;
	a.first = first; a.count = count; a.out_row0 = out_row0;
	a.means3D = b.means3D; a.shs = b.shs; a.colors_precomp = b.colors_precomp; a.scales = b.scales;
	a.scale_modifier = b.scale_modifier; a.rotations = b.rotations; a.cov3D_precomp = b.cov3D_precomp;
	a.viewmatrix = b.viewmatrix; a.projmatrix = b.projmatrix; a.cam_pos = b.cam_pos;
	a.tan_fovx = b.tan_fovx; a.tan_fovy = b.tan_fovy;
	a.focal_y = b.height / (2.0f * b.tan_fovy);
	a.focal_x = b.width / (2.0f * b.tan_fovx);
	if (o.cm) { a.focal_x = o.cm->fx; a.focal_y = o.cm->fy; }
	a.radii = b.radii; a.g = f.g;
	a.slots = f.slots; a.slot_valid = f.slot_valid;
	a.dL_dmean2D = b.dL_dmean2D; a.dL_dconic = b.dL_dconic; a.dL_dopacity = b.dL_dopacity; a.dL_dcolor = b.dL_dcolor;
	a.dL_dmean3D = b.dL_dmean3D; a.dL_dcov3D = b.dL_dcov3D; a.dL_dsh = b.dL_dsh; a.dL_dscale = b.dL_dscale; a.dL_drot = b.dL_drot;
	a.stat_xyz_gradient_accum = b.stat_xyz_gradient_accum; a.stat_denom = b.stat_denom; a.stat_max_radii2D = b.stat_max_radii2D;
	rc = gsr_stage(s, b.debug, "gaussian_backward", [&] { gsr_launch_gaussian_backward(a, s, o); });
	if (rc || !o.cam.rows) return rc;
	return fold((int)gsr_cam_rows(count));
}

extern "C" int gsr_backward_gaussians(const gsr_backward_args* args, int first, int count, int out_row0)
{
	return gsr_backward_gaussians_impl(args, first, count, out_row0, GsrGaussianOptions{});
}

// the option entry points: the one check under the caller's name, then the pass
static int gsr_backward_gaussians_opt(const char* who, bool aux_required, const gsr_backward_args* args, const gsr_camera_model* model, int antialiasing,
                                      const float* opacities, const gsr_aux_args* aux, const GsrCamTarget* cam, int first, int count, int out_row0)
{
	GsrGaussianOptions o;
	int rc;
	// (the per-Gaussian pass reads the mode of aux alone; the scratch's alignment is checked as the blend's call does)
	if ((rc = gsr_gaussian_options(&o, who, aux_required, GSR_AUX_NEEDS_SCRATCH, aux, antialiasing, opacities, model, cam, args, first, count))) return rc;
	return gsr_backward_gaussians_impl(args, first, count, out_row0, o);
}

extern "C" int gsr_backward_gaussians_aux(const gsr_backward_args* args, const gsr_aux_args* aux, int first, int count, int out_row0)
{
	return gsr_backward_gaussians_opt("gsr_backward_gaussians_aux", true, args, nullptr, 0, nullptr, aux, nullptr, first, count, out_row0);
}

extern "C" int gsr_backward_gaussians_aa(const gsr_backward_args* args, int antialiasing, const float* opacities, const gsr_aux_args* aux,
                                         int first, int count, int out_row0)
{
	return gsr_backward_gaussians_opt("gsr_backward_gaussians_aa", false, args, nullptr, antialiasing, opacities, aux, nullptr, first, count, out_row0);
}

// a camera model (include/gsr_camera_model.h): model NULL = gsr_backward_gaussians_aa
extern "C" int gsr_backward_gaussians_cm(const gsr_backward_args* args, const gsr_camera_model* model, int antialiasing, const float* opacities,
                                         const gsr_aux_args* aux, int first, int count, int out_row0)
{
	if (!model) return gsr_backward_gaussians_aa(args, antialiasing, opacities, aux, first, count, out_row0);
	return gsr_backward_gaussians_opt("gsr_backward_gaussians_cm", false, args, model, antialiasing, opacities, aux, nullptr, first, count, out_row0);
}

// ---- camera gradients (include/gsr_cam.h) ----
extern "C" size_t gsr_cam_bytes(int P) { return (gsr_cam_rows(P) > 0 ? gsr_cam_rows(P) : 1) * 32 * sizeof(float); }

extern "C" int gsr_backward_gaussians_cam(const gsr_backward_args* args, int antialiasing, const float* opacities, const gsr_aux_args* aux,
                                          const gsr_cam_args* cam, int first, int count, int out_row0)
{
	if (!cam) return gsr_backward_gaussians_aa(args, antialiasing, opacities, aux, first, count, out_row0);
	const GsrCamTarget t = {(float*)cam->scratch, cam->dL_dviewmatrix, cam->dL_dprojmatrix, cam->dL_dcampos};
	return gsr_backward_gaussians_opt("gsr_backward_gaussians_cam", false, args, nullptr, antialiasing, opacities, aux, &t, first, count, out_row0);
}

// ---- camera gradients under a camera model (include/gsr_cam_cm.h) ----
extern "C" size_t gsr_cam_cm_bytes(int P) { return gsr_cam_bytes(P); }   // the same rows of 32 floats, one per wave

extern "C" int gsr_backward_gaussians_cam_cm(const gsr_backward_args* args, const gsr_camera_model* model, int antialiasing,
                                             const float* opacities, const gsr_aux_args* aux, const gsr_cam_cm_args* cam, int first, int count,
                                             int out_row0)
{
	if (!cam) return gsr_backward_gaussians_cm(args, model, antialiasing, opacities, aux, first, count, out_row0);
	const char* who = "gsr_backward_gaussians_cam_cm";
	if (!model) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: the camera model is NULL (without one the camera gradients are gsr_backward_gaussians_cam's)", who);
	const GsrCamTarget t = {(float*)cam->scratch, cam->dL_dviewmatrix, cam->dL_dintrinsics, cam->dL_dcampos};
	return gsr_backward_gaussians_opt(who, false, args, model, antialiasing, opacities, aux, &t, first, count, out_row0);
}

static int gsr_backward_whole(const gsr_backward_args& a)
{
	int rc;
	if ((rc = gsr_backward_blend(&a))) return rc;
	return gsr_backward_gaussians(&a, 0, a.P, 0);
}

extern "C" int gsr_backward(int P, int D, int M, int64_t R, int width, int height, const float* background,
                            const float* means3D, const float* shs, const float* colors_precomp,
                            const float* scales, float scale_modifier, const float* rotations,
                            const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                            const float* cam_pos, float tan_fovx, float tan_fovy, const int* radii, void* geometry,
                            void* binning, void* image, void* scratch, const float* dL_dpix, float* dL_dmean2D,
                            float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                            float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, void* stream,
                            int debug)
{
	gsr_backward_args a = {};
	a.P = P; a.D = D; a.M = M; a.num_rendered = R; a.width = width; a.height = height; a.leaf = 0;
	a.background = background; a.means3D = means3D; a.shs = shs; a.colors_precomp = colors_precomp; a.scales = scales;
	a.scale_modifier = scale_modifier; a.rotations = rotations; a.cov3D_precomp = cov3D_precomp; a.viewmatrix = viewmatrix;
	a.projmatrix = projmatrix; a.cam_pos = cam_pos; a.tan_fovx = tan_fovx; a.tan_fovy = tan_fovy; a.radii = radii;
	a.geometry = geometry; a.binning = binning; a.image = image; a.scratch = scratch; a.dL_dpix = dL_dpix;
	a.dL_dmean2D = dL_dmean2D; a.dL_dconic = dL_dconic; a.dL_dopacity = dL_dopacity; a.dL_dcolor = dL_dcolor;
	a.dL_dmean3D = dL_dmean3D; a.dL_dcov3D = dL_dcov3D; a.dL_dsh = dL_dsh; a.dL_dscale = dL_dscale; a.dL_drot = dL_drot;
	a.stream = stream; a.debug = debug;
	return gsr_backward_whole(a);
}

extern "C" int gsr_backward_leaf(int P, int D, int M, int64_t R, int width, int height, const float* background,
                                 const float* xyz, const float* features_dc, const float* features_rest,
                                 const float* log_scales, float scale_modifier, const float* raw_rotations,
                                 const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                                 float tan_fovy, const int* radii, void* geometry, void* binning, void* image,
                                 void* scratch, const float* dL_dpix, float* dL_dmean2D, float* dL_dxyz,
                                 float* dL_dfeatures_dc, float* dL_dfeatures_rest, float* dL_dopacity_logits,
                                 float* dL_dlog_scales, float* dL_draw_rotations, float* dL_dRGB, void* stream, int debug)
{
	gsr_backward_args a = {};
	a.P = P; a.D = D; a.M = M; a.num_rendered = R; a.width = width; a.height = height; a.leaf = 1;
	a.background = background; a.means3D = xyz; a.shs = features_dc; a.shs_rest = features_rest; a.scales = log_scales;
	a.scale_modifier = scale_modifier; a.rotations = raw_rotations; a.viewmatrix = viewmatrix; a.projmatrix = projmatrix;
	a.cam_pos = cam_pos; a.tan_fovx = tan_fovx; a.tan_fovy = tan_fovy; a.radii = radii;
	a.geometry = geometry; a.binning = binning; a.image = image; a.scratch = scratch; a.dL_dpix = dL_dpix;
	a.dL_dmean2D = dL_dmean2D; a.dL_dopacity = dL_dopacity_logits; a.dL_dcolor = dL_dRGB; a.dL_dmean3D = dL_dxyz;
	a.dL_dsh = dL_dfeatures_dc; a.dL_dsh_rest = dL_dfeatures_rest; a.dL_dscale = dL_dlog_scales; a.dL_drot = dL_draw_rotations;
	a.stream = stream; a.debug = debug;
	return gsr_backward_whole(a);
}

// ---- absolute screen-space gradients (include/gsr_absgrad.h) -------------------------------------
extern "C" int gsr_backward_blend_abs(const gsr_backward_args* args, const gsr_aux_args* aux, int absgrad)
{
	if (absgrad != 0 && absgrad != 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward_blend_abs: absgrad must be 0 or 1, got %d", absgrad);
	int rc;
	if ((rc = gsr_option_check("gsr_backward_blend_abs", 0, aux, true, GSR_AUX_NEEDS_SCRATCH, args && args->P > 0 && args->num_rendered > 0))) return rc;
	return gsr_backward_blend_impl(args, aux, absgrad != 0);
}

extern "C" int gsr_absgrad_fold(const gsr_backward_args* args, const gsr_absgrad_args* abs, int first, int count)
{
	const char* who = "gsr_absgrad_fold";
	if (!args || !abs) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: args or abs is NULL", who);
	const gsr_backward_args& a = *args;
	int rc;
	if ((rc = gsr_frame_sizes(who, args))) return rc;
	if (first < 0 || count < 0 || (int64_t)first + count > a.P)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: bad range [%d, %d + %d) of %d Gaussians", who, first, first, count, a.P);
	if (!abs->abs_dL_dmean2D && !abs->stat_abs_gradient_accum)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: abs_dL_dmean2D and stat_abs_gradient_accum are both NULL", who);
	if (count == 0) return GSR_OK;
	GsrFrame f;
	if ((rc = gsr_frame_open(&f, who, GSR_FRAME_SLOTS, a, true))) return rc;
	return gsr_stage(f.s, f.debug, "absgrad_fold",
	                 [&] { gsr_launch_absgrad_fold(f, first, count, a.radii, abs->abs_dL_dmean2D, abs->stat_abs_gradient_accum); });
}

// ---- blend-weight statistics (include/gsr_contrib.h) --------------------------------------------
extern "C" size_t gsr_contrib_scratch_bytes(int P, int64_t R)
{
	(void)P;
	if (R < 0) return 0;
	return gsr_contrib_valid_offset(R) + gsr_align_up((size_t)R);   // the records, then one validity byte per slot
}

extern "C" int gsr_contributions(int P, int64_t R, int width, int height, const void* geometry, const void* binning, const void* image,
                                 const float* pixel_weight, float* weight_sum, float* weight_max, int32_t* pixel_count, void* scratch,
                                 void* stream, int debug)
{
	const char* who = "gsr_contributions";
	int rc;
	if ((rc = gsr_frame_sizes(who, P, R, width, height))) return rc;
	if (P == 0) return GSR_OK;   // (no Gaussian: an empty array's address means nothing)
	if (!weight_sum && !weight_max && !pixel_count) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: all three outputs are NULL", who);
	if (R > 0 && !scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: required pointer is NULL", who);
	GsrFrame f;
	if ((rc = gsr_frame_open(&f, who, GSR_FRAME_IMAGE | GSR_FRAME_R32, P, R, width, height, geometry, binning, image, nullptr, stream, debug,
	                         aligned16(scratch))))
		return rc;
	if (R == 0) return GSR_OK;   // nothing blended: every Gaussian is left untouched
	rc = gsr_stage(f.s, debug, "contrib_tiles", [&] {   // (with the clearing of the validity bytes: the caller's scratch may be uninitialised)
		const int e = gsr_check_hip(hipMemsetAsync((uint8_t*)scratch + gsr_contrib_valid_offset(R), 0, (size_t)R, f.s), "hipMemsetAsync(contrib validity)");
		if (!e) gsr_launch_contrib_tiles(f, pixel_weight, scratch);
		return e;
	});
	if (rc) return rc;
	return gsr_stage(f.s, debug, "contrib_gaussians", [&] { gsr_launch_contrib_gaussians(f, scratch, weight_sum, weight_max, pixel_count); });
}

// ---- blended feature channels (include/gsr_features.h) ---------------------------------------------
#define GSR_FEATURES_MAX_K (4 * 65535)   // one grid row of the tile passes per chunk of four channels

extern "C" size_t gsr_features_scratch_bytes(int P, int64_t R, int K)
{
	(void)P;
	if (R <= 0 || K < 1 || K > GSR_FEATURES_MAX_K) return 0;
	return gsr_features_valid_offset(R, K) + gsr_align_up((size_t)R);   // the records of every chunk, then one validity byte per slot
}

extern "C" int gsr_features_forward(int P, int64_t R, int width, int height, int K, const void* geometry, const void* binning, const void* image,
                                    const float* features, float* out, void* stream, int debug)
{
	const char* who = "gsr_features_forward";
	int rc;
	if ((rc = gsr_frame_sizes(who, P, R, width, height))) return rc;
	if (K < 1 || K > GSR_FEATURES_MAX_K) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: K must be in [1, %d], got %d", who, GSR_FEATURES_MAX_K, K);
	if (P == 0) return GSR_OK;   // (no Gaussian: an empty array's address means nothing)
	if (!features || !out) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: features or out is NULL", who);
	GsrFrame f;
	if ((rc = gsr_frame_open(&f, who, GSR_FRAME_IMAGE | GSR_FRAME_R32, P, R, width, height, geometry, binning, image, nullptr, stream, debug, true))) return rc;
	return gsr_stage(f.s, debug, "features_forward", [&] {
		if (R == 0)   // nothing blended: the map is zeros
			return gsr_check_hip(hipMemsetAsync(out, 0, (size_t)K * height * width * sizeof(float), f.s), "hipMemsetAsync(feature map)");
		gsr_launch_features_forward(f, K, features, out);
		return (int)GSR_OK;
	});
}

extern "C" int gsr_features_backward(const gsr_backward_args* args, int K, const float* features, const float* dL_dout, float* dL_dfeatures,
                                     void* scratch, int into_slots)
{
	const char* who = "gsr_features_backward";
	int rc;
	if ((rc = gsr_frame_sizes(who, args))) return rc;
	const gsr_backward_args& a = *args;
	const int64_t R = a.num_rendered;
	if (K < 1 || K > GSR_FEATURES_MAX_K) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: K must be in [1, %d], got %d", who, GSR_FEATURES_MAX_K, K);
	if (into_slots != 0 && into_slots != 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: into_slots must be 0 or 1, got %d", who, into_slots);
	if (a.P == 0) return GSR_OK;
	if (!features || !dL_dout || !dL_dfeatures) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: features, dL_dout or dL_dfeatures is NULL", who);
	if (R > 0 && !scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: required pointer is NULL", who);
	GsrFrame f;   // (into_slots = 0: the slots are neither needed nor passed on)
	if ((rc = gsr_frame_open(&f, who, GSR_FRAME_IMAGE | GSR_FRAME_R32 | (into_slots ? GSR_FRAME_SLOTS : 0), a, aligned16(scratch)))) return rc;
	if (R == 0)   // nothing blended: every gradient is zero
		return gsr_stage(f.s, f.debug, "features_backward_fold", [&] {
			return gsr_check_hip(hipMemsetAsync(dL_dfeatures, 0, (size_t)a.P * K * sizeof(float), f.s), "hipMemsetAsync(dL_dfeatures)");
		});
	rc = gsr_stage(f.s, f.debug, "features_backward_tiles", [&] {   // (with the clearing of the validity bytes: the caller's scratch may be uninitialised)
		const int e = gsr_check_hip(hipMemsetAsync((uint8_t*)scratch + gsr_features_valid_offset(R, K), 0, (size_t)R, f.s), "hipMemsetAsync(features validity)");
		if (!e) gsr_launch_features_backward_tiles(f, K, features, dL_dout, scratch);
		return e;
	});
	if (rc) return rc;
	return gsr_stage(f.s, f.debug, "features_backward_fold", [&] { gsr_launch_features_fold(f, K, scratch, dL_dfeatures); });
}

// ---- depth-distortion map (include/gsr_distortion.h) ------------------------------------------------
extern "C" size_t gsr_distortion_state_bytes(int width, int height)
{
	if (width <= 0 || height <= 0) return 0;
	return gsr_align_up((size_t)3 * (size_t)width * (size_t)height * sizeof(float));   // the planes A, mu, S
}

extern "C" int gsr_distortion_forward(int P, int64_t R, int width, int height, const void* geometry, const void* binning, const void* image,
                                      float* out_dist, void* state, void* stream, int debug)
{
	const char* who = "gsr_distortion_forward";
	int rc;
	if ((rc = gsr_frame_sizes(who, P, R, width, height))) return rc;
	if (P == 0) return GSR_OK;   // (no Gaussian: an empty array's address means nothing)
	if (!out_dist || !state) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: out_dist or state is NULL", who);
	GsrFrame f;
	if ((rc = gsr_frame_open(&f, who, GSR_FRAME_IMAGE | GSR_FRAME_R32, P, R, width, height, geometry, binning, image, nullptr, stream, debug,
	                         aligned16(state))))
		return rc;
	return gsr_stage(f.s, debug, "distortion_forward", [&] {
		if (R == 0) {   // nothing blended: the map and the state are zeros
			const size_t plane = (size_t)height * width * sizeof(float);
			if (int e = gsr_check_hip(hipMemsetAsync(out_dist, 0, plane, f.s), "hipMemsetAsync(distortion map)")) return e;
			return gsr_check_hip(hipMemsetAsync(state, 0, 3 * plane, f.s), "hipMemsetAsync(distortion state)");
		}
		gsr_launch_distortion_forward(f, out_dist, (float*)state);
		return (int)GSR_OK;
	});
}

extern "C" int gsr_distortion_backward(const gsr_backward_args* args, const void* state, const float* dL_ddist)
{
	const char* who = "gsr_distortion_backward";
	int rc;
	if ((rc = gsr_frame_sizes(who, args))) return rc;
	if (args->P == 0) return GSR_OK;
	if (!state || !dL_ddist) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: state or dL_ddist is NULL", who);
	GsrFrame f;
	if ((rc = gsr_frame_open(&f, who, GSR_FRAME_IMAGE | GSR_FRAME_SLOTS | GSR_FRAME_R32, *args, aligned16(state)))) return rc;
	if (f.R == 0) return GSR_OK;   // nothing blended: no slot to add into
	return gsr_stage(f.s, f.debug, "distortion_backward", [&] { gsr_launch_distortion_backward(f, (const float*)state, dL_ddist); });
}

// ---- median-depth and per-pixel index maps (include/gsr_median.h) -----------------------------------
extern "C" size_t gsr_median_state_bytes(int width, int height)
{
	if (width <= 0 || height <= 0) return 0;
	return gsr_align_up((size_t)width * (size_t)height * sizeof(uint32_t));   // the median's list position per pixel
}

extern "C" int gsr_median_forward(int P, int64_t R, int width, int height, const void* geometry, const void* binning, const void* image,
                                  float* out_median_depth, int32_t* out_median_index, int32_t* out_dominant_index, float* out_dominant_weight,
                                  void* state, void* stream, int debug)
{
	const char* who = "gsr_median_forward";
	int rc;
	if ((rc = gsr_frame_sizes(who, P, R, width, height))) return rc;
	if (P == 0) return GSR_OK;   // (no Gaussian: an empty array's address means nothing)
	if (!out_median_depth && !out_median_index && !out_dominant_index && !out_dominant_weight)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: every output is NULL", who);
	if (out_median_depth && !state) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: out_median_depth needs state", who);
	GsrFrame f;
	if ((rc = gsr_frame_open(&f, who, GSR_FRAME_IMAGE | GSR_FRAME_R32, P, R, width, height, geometry, binning, image, nullptr, stream, debug,
	                         aligned16(state))))
		return rc;
	return gsr_stage(f.s, debug, "median_forward", [&] {
		if (R == 0) {   // nothing blended: depth and weight 0, indices -1, no position in the state
			const size_t plane = (size_t)height * width * 4;
			void* const outs[5] = {out_median_depth, out_dominant_weight, out_median_index, out_dominant_index, state};
			for (int i = 0; i < 5; i++)
				if (outs[i])
					if (int e = gsr_check_hip(hipMemsetAsync(outs[i], i < 2 ? 0 : 0xFF, plane, f.s), "hipMemsetAsync(median maps)")) return e;
			return (int)GSR_OK;
		}
		gsr_launch_median_forward(f, out_median_depth, out_median_index, out_dominant_index, out_dominant_weight, (uint32_t*)state,
		                          (debug & GSR_DEBUG_MEDIAN_FULL_WALK) != 0);
		return (int)GSR_OK;
	});
}

extern "C" int gsr_median_backward(const gsr_backward_args* args, const void* state, const float* dL_dmedian)
{
	const char* who = "gsr_median_backward";
	int rc;
	if ((rc = gsr_frame_sizes(who, args))) return rc;
	if (args->P == 0) return GSR_OK;
	if (!state || !dL_dmedian) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: state or dL_dmedian is NULL", who);
	GsrFrame f;
	if ((rc = gsr_frame_open(&f, who, GSR_FRAME_IMAGE | GSR_FRAME_SLOTS | GSR_FRAME_R32, *args, aligned16(state)))) return rc;
	if (f.R == 0) return GSR_OK;   // nothing blended: no slot to add into
	return gsr_stage(f.s, f.debug, "median_backward", [&] { gsr_launch_median_backward(f, (const uint32_t*)state, dL_dmedian); });
}

// ---- per-Gaussian normals, depth normals and the normal-consistency loss (include/gsr_normals.h) ----
static int gsr_gaussian_normals_check(const char* who, int P, const void* scales, const void* rotations, const void* means3D,
                                      const void* viewmatrix, int space, const void* in, const void* out)
{
	if (P < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: negative P (%d)", who, P);
	if (space != GSR_NORMALS_VIEW && space != GSR_NORMALS_WORLD)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: space must be GSR_NORMALS_VIEW or GSR_NORMALS_WORLD (got %d)", who, space);
	if (P == 0) return GSR_OK;
	if (!scales || !rotations || !means3D || !viewmatrix || !in || !out) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: NULL pointer", who);
	if (!aligned16(rotations)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: rotations must be 16-byte aligned", who);
	return GSR_OK;
}

extern "C" int gsr_gaussian_normals(int P, const float* scales, const float* rotations, const float* means3D, const float* viewmatrix,
                                    int space, float* out, void* stream)
{
	g_err[0] = 0;
	const int rc = gsr_gaussian_normals_check("gsr_gaussian_normals", P, scales, rotations, means3D, viewmatrix, space, scales, out);
	if (rc != GSR_OK || P == 0) return rc;
	gsr_launch_gaussian_normals(P, scales, rotations, means3D, viewmatrix, space == GSR_NORMALS_WORLD, out, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "gaussian_normals");
}

extern "C" int gsr_gaussian_normals_backward(int P, const float* scales, const float* rotations, const float* means3D, const float* viewmatrix,
                                             int space, const float* dL_dout, float* dL_drotations, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_gaussian_normals_backward";
	const int rc = gsr_gaussian_normals_check(who, P, scales, rotations, means3D, viewmatrix, space, dL_dout, dL_drotations);
	if (rc != GSR_OK || P == 0) return rc;
	if (!aligned16(dL_drotations)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: dL_drotations must be 16-byte aligned", who);
	gsr_launch_gaussian_normals_backward(P, scales, rotations, means3D, viewmatrix, space == GSR_NORMALS_WORLD, dL_dout, dL_drotations,
	                                     (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "gaussian_normals_backward");
}

extern "C" size_t gsr_normals_scratch_bytes(int W, int H)
{
	if (W <= 0 || H <= 0) return 0;
	return gsr_normals_scratch_size(W, H);
}

extern "C" int gsr_depth_normals(int W, int H, const float* depth, float tanfovx, float tanfovy, float* out, void* stream)
{
	g_err[0] = 0;
	if (W <= 0 || H <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_depth_normals: bad image size (%d x %d)", W, H);
	if (!depth || !out) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_depth_normals: NULL pointer");
	gsr_launch_depth_normals(W, H, depth, tanfovx, tanfovy, out, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "depth_normals");
}

extern "C" int gsr_depth_normals_backward(int W, int H, const float* depth, float tanfovx, float tanfovy, const float* dL_dout,
                                          float* dL_ddepth, void* stream)
{
	g_err[0] = 0;
	if (W <= 0 || H <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_depth_normals_backward: bad image size (%d x %d)", W, H);
	if (!depth || !dL_dout || !dL_ddepth) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_depth_normals_backward: NULL pointer");
	gsr_launch_depth_normals_backward(W, H, depth, tanfovx, tanfovy, dL_dout, dL_ddepth, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "depth_normals_backward");
}

extern "C" int gsr_normal_consistency_loss(int W, int H, const float* normal_map, const float* depth, const float* alpha, float tanfovx,
                                           float tanfovy, float* vals, float* dL_dnormal_map, float* dL_ddepth, void* scratch, void* stream)
{
	g_err[0] = 0;
	if (W <= 0 || H <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_normal_consistency_loss: bad image size (%d x %d)", W, H);
	if (!normal_map || !depth || !vals || !scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_normal_consistency_loss: NULL pointer");
	gsr_launch_normal_consistency_loss(W, H, normal_map, depth, alpha, tanfovx, tanfovy, vals, dL_dnormal_map, dL_ddepth, scratch,
	                                   (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "normal_consistency_loss");
}

extern "C" size_t gsr_loss_scratch_bytes(int C, int H, int W)
{
	if (C <= 0 || H <= 0 || W <= 0) return 0;
	size_t a, b;
	int n;
	return gsr_loss_scratch_layout(C, H, W, &a, &b, &n);
}

extern "C" int gsr_l1_ssim_loss(int C, int H, int W, const float* img, const float* gt, float lambda_dssim, float* loss_out,
                                float* dL_dimg, void* scratch, void* stream)
{
	g_err[0] = 0;
	if (C <= 0 || H <= 0 || W <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_l1_ssim_loss: bad image size");
	if (!img || !gt || !loss_out || !scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_l1_ssim_loss: NULL pointer");
	gsr_launch_l1_ssim(C, H, W, img, gt, lambda_dssim, loss_out, dL_dimg, scratch, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "l1_ssim_loss");
}

// ---- the fused loss with a pixel mask, an exposure and an inverse-depth term (include/gsr_loss_ext.h) ----
extern "C" size_t gsr_loss_ext_scratch_bytes(int C, int H, int W)
{
	if (C <= 0 || H <= 0 || W <= 0) return 0;
	size_t a, b, c;
	int n, nxy;
	return gsr_loss_ext_scratch_layout(C, H, W, &a, &b, &c, &n, &nxy);
}

extern "C" int gsr_l1_ssim_loss_ext(const gsr_loss_ext_args* args)
{
	g_err[0] = 0;
	const char* who = "gsr_l1_ssim_loss_ext";
	if (!args) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: NULL args", who);
	const gsr_loss_ext_args& a = *args;
	if (a.C <= 0 || a.H <= 0 || a.W <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: bad image size (%d x %d x %d)", who, a.C, a.H, a.W);
	if (!a.img || !a.gt || !a.vals || !a.scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: NULL pointer", who);
	if (a.exposure && a.C != 3) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: exposure needs C == 3 (got %d)", who, a.C);
	if (a.dL_dexposure && !a.exposure) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: dL_dexposure without exposure", who);
	if (!a.invdepth != !a.invdepth_prior) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: invdepth and invdepth_prior go together", who);
	if (!a.invdepth && (a.invdepth_mask || a.dL_dinvdepth))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: invdepth_mask / dL_dinvdepth without invdepth and invdepth_prior", who);
	if (!(a.invdepth_weight >= 0.f) || !std::isfinite(a.invdepth_weight))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: invdepth_weight must be finite and >= 0", who);
	gsr_launch_l1_ssim_ext(a, (hipStream_t)a.stream);
	return gsr_stage_done((hipStream_t)a.stream, 0, "l1_ssim_loss_ext");
}

// ---- the bilateral grid of affine colour transforms (include/gsr_bilagrid.h) ----
#define GSR_BILAGRID_MAX_BLOCKS ((1LL << 24) - 1)   // workgroups of 256 threads in one launch

static bool gsr_bilagrid_sizes_ok(int H, int W, int L, int GH, int GW)
{
	return H >= 1 && W >= 1 && L >= 2 && GH >= 2 && GW >= 2;
}
// the kernels index pixels and grid entries with 32 bits
static bool gsr_bilagrid_fits(long long count, int a, int b, int c) { return (double)count * a * b * c <= 2147483647.0; }

static int gsr_bilagrid_check(const char* who, const gsr_bilagrid_args* args)
{
	if (!args) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: NULL args", who);
	const gsr_bilagrid_args& a = *args;
	if (a.H < 1 || a.W < 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: bad image size (%d x %d)", who, a.H, a.W);
	if (a.L < 2 || a.GH < 2 || a.GW < 2)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: every grid axis must be at least 2 (got L %d, GH %d, GW %d)", who, a.L, a.GH, a.GW);
	if (!gsr_bilagrid_fits(3, a.H, a.W, 1) || !gsr_bilagrid_fits(12, a.L, a.GH, a.GW))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: the image or the grid exceeds 32-bit indexing", who);
	if (gsr_bilagrid_tiles(a.H, a.W) > GSR_BILAGRID_MAX_BLOCKS || gsr_bilagrid_gather_blocks(a.H, a.L, a.GH, a.GW) > GSR_BILAGRID_MAX_BLOCKS)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: the image or the grid needs more than 2^24 - 1 workgroups", who);
	if (!a.grid || !a.img) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: grid or img is NULL", who);
	return GSR_OK;
}

extern "C" size_t gsr_bilagrid_scratch_bytes(int H, int W, int L, int GH, int GW)
{
	if (!gsr_bilagrid_sizes_ok(H, W, L, GH, GW) || !gsr_bilagrid_fits(3, H, W, 1) || !gsr_bilagrid_fits(12, L, GH, GW)) return 0;
	return gsr_bilagrid_scratch_size(H, W, L, GH, GW);
}

extern "C" int gsr_bilagrid_slice(const gsr_bilagrid_args* args)
{
	g_err[0] = 0;
	const char* who = "gsr_bilagrid_slice";
	const int rc = gsr_bilagrid_check(who, args);
	if (rc != GSR_OK) return rc;
	if (!args->out) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: out is NULL", who);
	gsr_launch_bilagrid_slice(*args, (hipStream_t)args->stream);
	return gsr_stage_done((hipStream_t)args->stream, 0, "bilagrid_slice");
}

extern "C" int gsr_bilagrid_slice_backward(const gsr_bilagrid_args* args)
{
	g_err[0] = 0;
	const char* who = "gsr_bilagrid_slice_backward";
	const int rc = gsr_bilagrid_check(who, args);
	if (rc != GSR_OK) return rc;
	const gsr_bilagrid_args& a = *args;
	if (!a.dL_dout) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: dL_dout is NULL", who);
	if (!a.dL_dgrid && !a.dL_dimg) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: dL_dgrid and dL_dimg are both NULL", who);
	if (a.dL_dgrid && !a.scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: scratch is NULL", who);
	gsr_launch_bilagrid_backward(a, (hipStream_t)a.stream);
	return gsr_stage_done((hipStream_t)a.stream, 0, "bilagrid_backward");
}

extern "C" size_t gsr_bilagrid_tv_scratch_bytes(int N, int L, int GH, int GW)
{
	if (N < 1 || L < 2 || GH < 2 || GW < 2 || !gsr_bilagrid_fits(12LL * N, L, GH, GW)) return 0;
	return gsr_bilagrid_tv_scratch_size(N, L, GH, GW);
}

extern "C" int gsr_bilagrid_tv(int N, int L, int GH, int GW, const float* grids, float* val, float* dL_dgrids, void* scratch, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_bilagrid_tv";
	if (N < 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: N must be at least 1 (got %d)", who, N);
	if (L < 2 || GH < 2 || GW < 2)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: every grid axis must be at least 2 (got L %d, GH %d, GW %d)", who, L, GH, GW);
	if (!gsr_bilagrid_fits(12LL * N, L, GH, GW)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: the grids exceed 32-bit indexing", who);
	if (!grids || !val || !scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: grids, val or scratch is NULL", who);
	gsr_launch_bilagrid_tv(N, L, GH, GW, grids, val, dL_dgrids, scratch, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "bilagrid_tv");
}

// ---- fixed-budget (MCMC) training: noise injection, relocation, regulariser (include/gsr_mcmc.h) ----
#define GSR_MCMC_MAX_BLOCKS ((1LL << 24) - 1)   // workgroups in one launch; only D can ask for more (P is held below by the 32-bit indices)
// the kernels index every tensor with 32 bits
static bool gsr_mcmc_fits(long long rows, long long row) { return (double)rows * (double)row <= 2147483647.0; }

extern "C" int gsr_mcmc_noise(int P, float* xyz, const float* opacity, const float* scaling, const float* rotation, const float* noise,
                              float scaler, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_mcmc_noise";
	if (P < 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: P must be at least 1 (got %d)", who, P);
	if (!gsr_mcmc_fits(P, 4)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: 4 P exceeds 32-bit indexing (P %d)", who, P);
	if (!xyz || !opacity || !scaling || !rotation || !noise)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: xyz, opacity, scaling, rotation or noise is NULL", who);
	gsr_launch_mcmc_noise(P, xyz, opacity, scaling, rotation, noise, scaler, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "mcmc_noise");
}

extern "C" int gsr_mcmc_relocate(const gsr_mcmc_relocate_args* args)
{
	g_err[0] = 0;
	const char* who = "gsr_mcmc_relocate";
	if (!args) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: NULL args", who);
	const gsr_mcmc_relocate_args& a = *args;
	if (a.P < 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: P must be at least 1 (got %d)", who, a.P);
	if (a.D < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: negative entry count (D %d)", who, a.D);
	if (a.ngroups < 1 || a.ngroups > GSR_ADAM_MAX_GROUPS) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: 1..%d groups (got %d)", who, GSR_ADAM_MAX_GROUPS, a.ngroups);
	if (!a.groups) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: groups is NULL", who);
	if (a.opacity_group < 0 || a.opacity_group >= a.ngroups || a.scale_group < 0 || a.scale_group >= a.ngroups || a.opacity_group == a.scale_group)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: opacity_group %d and scale_group %d must be two of the %d groups", who, a.opacity_group, a.scale_group,
		                a.ngroups);
	for (int k = 0; k < a.ngroups; k++) {
		const gsr_mcmc_group& g = a.groups[k];
		if (g.row < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d: negative row", who, k);
		if (g.row > 0 && !g.param) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d: param is NULL", who, k);
		if ((g.exp_avg != nullptr) != (g.exp_avg_sq != nullptr))
			return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d: exp_avg and exp_avg_sq go together", who, k);
		if (!gsr_mcmc_fits(a.P, g.row)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d exceeds 32-bit indexing (P %d, row %d)", who, k, a.P, g.row);
	}
	if (a.groups[a.opacity_group].row != 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: the opacity group's row must be 1 (got %d)", who, a.groups[a.opacity_group].row);
	if (a.groups[a.scale_group].row != 3) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: the scale group's row must be 3 (got %d)", who, a.groups[a.scale_group].row);
	if (!(a.min_opacity > 0.0f && a.min_opacity < 1.0f)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: min_opacity must lie in (0, 1) (got %g)", who, (double)a.min_opacity);
	if (gsr_mcmc_relocate_blocks(a.D) > GSR_MCMC_MAX_BLOCKS) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: D needs more than 2^24 - 1 workgroups (D %d)", who, a.D);
	if (a.D == 0) return GSR_OK;   // nothing to launch
	if (!a.dst || !a.src || !a.counts) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: dst, src or counts is NULL", who);
	const int rc = gsr_launch_mcmc_relocate(a, (hipStream_t)a.stream);
	if (rc != GSR_OK) return rc;
	return gsr_stage_done((hipStream_t)a.stream, 0, "mcmc_relocate");
}

extern "C" size_t gsr_mcmc_regularizer_scratch_bytes(int P)
{
	if (P < 1 || !gsr_mcmc_fits(P, 3)) return 0;
	return gsr_mcmc_reg_scratch_size(P);
}

extern "C" int gsr_mcmc_regularizer(int P, const float* opacity, const float* scaling, float w_o, float w_s, float* val, float* dL_dopacity,
                                    float* dL_dscaling, void* scratch, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_mcmc_regularizer";
	if (P < 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: P must be at least 1 (got %d)", who, P);
	if (!gsr_mcmc_fits(P, 3)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: 3 P exceeds 32-bit indexing (P %d)", who, P);
	if (!opacity || !scaling || !val || !scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: opacity, scaling, val or scratch is NULL", who);
	gsr_launch_mcmc_regularizer(P, opacity, scaling, w_o, w_s, val, dL_dopacity, dL_dscaling, scratch, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "mcmc_reg");
}

// ---- densification: clone, split and prune as one compaction (include/gsr_densify.h) ----
extern "C" size_t gsr_densify_scratch_bytes(int P)
{
	if (P < 1) return 0;
	return gsr_densify_scratch_size(P);
}

extern "C" int gsr_densify_plan(int P, const uint8_t* action, void* scratch, int32_t* totals, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_densify_plan";
	if (P < 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: P must be at least 1 (got %d)", who, P);
	if (!action || !scratch || !totals) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: action, scratch or totals is NULL", who);
	if (gsr_densify_plan_blocks(P) > GSR_MCMC_MAX_BLOCKS) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: P needs more than 2^24 - 1 workgroups (P %d)", who, P);
	gsr_launch_densify_plan(P, action, scratch, totals, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "densify_plan");
}

extern "C" int gsr_densify_apply(const gsr_densify_args* args)
{
	g_err[0] = 0;
	const char* who = "gsr_densify_apply";
	if (!args) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: NULL args", who);
	const gsr_densify_args& a = *args;
	if (a.P < 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: P must be at least 1 (got %d)", who, a.P);
	if (a.K < 0 || a.C < 0 || a.S < 0 || a.C > a.K || (long long)a.K + a.S > a.P)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: K %d, C %d, S %d are no counts over %d rows (0 <= C <= K, 0 <= S, K + S <= P)", who, a.K, a.C, a.S, a.P);
	if (a.ngroups < 1 || a.ngroups > GSR_DENSIFY_MAX_GROUPS) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: 1..%d groups (got %d)", who, GSR_DENSIFY_MAX_GROUPS, a.ngroups);
	if (!a.groups) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: groups is NULL", who);
	const long long Pout = (long long)a.K + a.C + (long long)GSR_DENSIFY_SPLIT_N * a.S;
	for (int k = 0; k < a.ngroups; k++) {
		const gsr_densify_group& g = a.groups[k];
		if (g.row < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d: negative row", who, k);
		if ((g.exp_avg != nullptr) != (g.exp_avg_sq != nullptr))
			return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d: exp_avg and exp_avg_sq go together", who, k);
		if (!gsr_mcmc_fits(a.P, g.row) || !gsr_mcmc_fits(Pout, g.row))
			return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d exceeds 32-bit indexing (P %d, P' %lld, row %d)", who, k, a.P, Pout, g.row);
		if (gsr_densify_copy_blocks(Pout * g.row) > GSR_MCMC_MAX_BLOCKS)
			return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d needs more than 2^24 - 1 workgroups", who, k);
		if (g.row == 0) continue;
		if (!g.param) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d: param is NULL", who, k);
		if (Pout > 0 && (!g.out_param || (g.exp_avg && (!g.out_exp_avg || !g.out_exp_avg_sq))))
			return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d: an output is NULL", who, k);
	}
	const int named[3] = {a.xyz_group, a.scale_group, a.rotation_group}, want[3] = {3, 3, 4};
	const char* const label[3] = {"xyz_group", "scale_group", "rotation_group"};
	for (int n = 0; n < 3; n++) {
		if (named[n] == -1 && a.S == 0) continue;
		if (named[n] < 0 || named[n] >= a.ngroups)
			return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: %s %d names none of the %d groups%s", who, label[n], named[n], a.ngroups, a.S > 0 ? " (needed with S > 0)" : "");
		for (int m = 0; m < n; m++)
			if (named[m] == named[n]) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: %s and %s are one group (%d)", who, label[m], label[n], named[n]);
		if (a.groups[named[n]].row != want[n])
			return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: the row of %s must be %d (got %d)", who, label[n], want[n], a.groups[named[n]].row);
	}
	if (gsr_densify_plan_blocks(a.P) > GSR_MCMC_MAX_BLOCKS) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: P needs more than 2^24 - 1 workgroups (P %d)", who, a.P);
	if (!a.action || !a.scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: action or scratch is NULL", who);
	if (a.S > 0 && !a.noise) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: noise is NULL with S > 0", who);
	if (Pout == 0) return GSR_OK;   // nothing to write
	if (!a.src_of) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: src_of is NULL", who);
	gsr_launch_densify_apply(a, (hipStream_t)a.stream);
	return gsr_stage_done((hipStream_t)a.stream, 0, "densify_apply");
}

// ---- Mip-Splatting's 3D smoothing filter: camera sweep, filtered activations, baked leaves, reset (include/gsr_filter3d.h) ----
// what every entry point refuses about P; 0 where there is nothing to refuse
static int gsr_filter3d_size(const char* who, int P)
{
	if (P < 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: P must be at least 1 (got %d)", who, P);
	if (!gsr_mcmc_fits(P, 3)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: 3 P exceeds 32-bit indexing (P %d)", who, P);
	return GSR_OK;
}

extern "C" size_t gsr_filter3d_scratch_bytes(int P)
{
	if (P < 1 || !gsr_mcmc_fits(P, 3)) return 0;
	return gsr_filter3d_scratch_size(P);
}

extern "C" int gsr_filter3d_compute(int P, int C, const float* xyz, const gsr_filter3d_camera* cameras, int per_camera, float* filter, void* scratch,
                                    void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_filter3d_compute";
	if (const int rc = gsr_filter3d_size(who, P)) return rc;
	if (C < 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: C must be at least 1 (got %d)", who, C);
	if (!xyz || !cameras || !filter || !scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: xyz, cameras, filter or scratch is NULL", who);
	gsr_launch_filter3d_sweep(P, C, xyz, cameras, per_camera != 0, filter, scratch, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "filter3d_sweep");
}

static int gsr_filter3d_forward(const char* who, int P, const float* opacity, const float* scaling, const float* filter, float* out_o, float* out_s,
                                int baked, void* stream)
{
	g_err[0] = 0;
	if (const int rc = gsr_filter3d_size(who, P)) return rc;
	if (!opacity || !scaling || !filter) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: opacity, scaling or filter is NULL", who);
	if (!out_o && !out_s) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: both outputs are NULL", who);
	gsr_launch_filter3d_activate(P, opacity, scaling, filter, out_o, out_s, baked, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "filter3d_activate");
}

extern "C" int gsr_filter3d_activate(int P, const float* opacity, const float* scaling, const float* filter, float* opacities, float* scales,
                                     void* stream)
{
	return gsr_filter3d_forward("gsr_filter3d_activate", P, opacity, scaling, filter, opacities, scales, 0, stream);
}

extern "C" int gsr_filter3d_bake(int P, const float* opacity, const float* scaling, const float* filter, float* logits, float* log_scales,
                                 void* stream)
{
	return gsr_filter3d_forward("gsr_filter3d_bake", P, opacity, scaling, filter, logits, log_scales, 1, stream);
}

extern "C" int gsr_filter3d_activate_backward(int P, const float* opacity, const float* scaling, const float* filter, const float* dL_dopacities,
                                              const float* dL_dscales, float* dL_dopacity, float* dL_dscaling, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_filter3d_activate_backward";
	if (const int rc = gsr_filter3d_size(who, P)) return rc;
	if (!opacity || !scaling || !filter) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: opacity, scaling or filter is NULL", who);
	if (!dL_dopacity && !dL_dscaling) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: both outputs are NULL", who);
	gsr_launch_filter3d_activate_backward(P, opacity, scaling, filter, dL_dopacities, dL_dscales, dL_dopacity, dL_dscaling, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "filter3d_activate_bwd");
}

extern "C" int gsr_filter3d_reset_opacity(int P, float* opacity, const float* scaling, const float* filter, double max_opacity, float* exp_avg,
                                          float* exp_avg_sq, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_filter3d_reset_opacity";
	if (const int rc = gsr_filter3d_size(who, P)) return rc;
	if (!opacity || !scaling || !filter) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: opacity, scaling or filter is NULL", who);
	if ((exp_avg != nullptr) != (exp_avg_sq != nullptr)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: exp_avg and exp_avg_sq go together", who);
	if (!(max_opacity > 0.0 && max_opacity < 1.0)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: max_opacity must lie in (0, 1) (got %g)", who, max_opacity);
	gsr_launch_filter3d_reset(P, opacity, scaling, filter, max_opacity, exp_avg, exp_avg_sq, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "filter3d_reset");
}

// ---- 4D Gaussians at a time stamp: the slice and the harmonic colour coefficients (include/gsr_slice4d.h) ----
// what every entry point refuses about P; 0 where there is nothing to refuse
static int gsr_slice4d_size(const char* who, int P)
{
	if (P < 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: P must be at least 1 (got %d)", who, P);
	if (!gsr_mcmc_fits(P, 6)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: 6 P exceeds 32-bit indexing (P %d)", who, P);
	return GSR_OK;
}

// ... and about the leaves and the two scalars of the slice
static int gsr_slice4d_inputs(const char* who, int P, const float* xyz, const float* t, const float* scaling, const float* scaling_t,
                              const float* rotation, const float* rotation_r, const float* opacity, double modifier, double cutoff)
{
	if (const int rc = gsr_slice4d_size(who, P)) return rc;
	if (!xyz || !t || !scaling || !scaling_t || !rotation || !rotation_r || !opacity)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: xyz, t, scaling, scaling_t, rotation, rotation_r or opacity is NULL", who);
	if (!(std::isfinite(modifier) && modifier > 0.0))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: scaling_modifier must be finite and positive (got %g)", who, modifier);
	if (!(cutoff >= 0.0 && cutoff < 1.0)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: cutoff must lie in [0, 1) (got %g)", who, cutoff);
	return GSR_OK;
}

extern "C" int gsr_slice4d_forward(int P, const float* xyz, const float* t, const float* scaling, const float* scaling_t, const float* rotation,
                                   const float* rotation_r, const float* opacity, double time, double scaling_modifier, double cutoff, float* means3D,
                                   float* cov3D, float* opacities, float* velocity, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_slice4d_forward";
	if (const int rc = gsr_slice4d_inputs(who, P, xyz, t, scaling, scaling_t, rotation, rotation_r, opacity, scaling_modifier, cutoff)) return rc;
	if (!means3D && !cov3D && !opacities && !velocity) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: every output is NULL", who);
	gsr_launch_slice4d_forward(P, xyz, t, scaling, scaling_t, rotation, rotation_r, opacity, time, scaling_modifier, cutoff, means3D, cov3D, opacities,
	                           velocity, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "slice4d_forward");
}

extern "C" int gsr_slice4d_backward(int P, const float* xyz, const float* t, const float* scaling, const float* scaling_t, const float* rotation,
                                    const float* rotation_r, const float* opacity, double time, double scaling_modifier, double cutoff,
                                    const float* dL_dmeans3D, const float* dL_dcov3D, const float* dL_dopacities, const float* dL_dvelocity,
                                    float* dL_dxyz, float* dL_dt, float* dL_dscaling, float* dL_dscaling_t, float* dL_drotation, float* dL_drotation_r,
                                    float* dL_dopacity, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_slice4d_backward";
	if (const int rc = gsr_slice4d_inputs(who, P, xyz, t, scaling, scaling_t, rotation, rotation_r, opacity, scaling_modifier, cutoff)) return rc;
	if (!dL_dxyz && !dL_dt && !dL_dscaling && !dL_dscaling_t && !dL_drotation && !dL_drotation_r && !dL_dopacity)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: every output is NULL", who);
	gsr_slice4d_backward_args a;
	a.P = P;
	a.xyz = xyz; a.t = t; a.scaling = scaling; a.scaling_t = scaling_t; a.rotation = rotation; a.rotation_r = rotation_r; a.opacity = opacity;
	a.time = time; a.modifier = scaling_modifier; a.cutoff = cutoff;
	a.g_means3D = dL_dmeans3D; a.g_cov3D = dL_dcov3D; a.g_opacities = dL_dopacities; a.g_velocity = dL_dvelocity;
	a.d_xyz = dL_dxyz; a.d_t = dL_dt; a.d_scaling = dL_dscaling; a.d_scaling_t = dL_dscaling_t; a.d_rotation = dL_drotation;
	a.d_rotation_r = dL_drotation_r; a.d_opacity = dL_dopacity;
	gsr_launch_slice4d_backward(a, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "slice4d_backward");
}

// what both harmonic entry points refuse about their sizes and the period
static int gsr_harmonic_inputs(const char* who, int P, int N, int M, const float* features_t, const float* t, double period)
{
	if (const int rc = gsr_slice4d_size(who, P)) return rc;
	if (N < 0 || N > GSR_HARMONIC_MAX_N) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: N must lie in 0..%d (got %d)", who, GSR_HARMONIC_MAX_N, N);
	if (M < 1 || M > GSR_HARMONIC_MAX_M) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: M must lie in 1..%d (got %d)", who, GSR_HARMONIC_MAX_M, M);
	if (!features_t || !t) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: features_t or t is NULL", who);
	if (!(std::isfinite(period) && period > 0.0)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: period must be finite and positive (got %g)", who, period);
	return GSR_OK;
}

extern "C" int gsr_harmonic_features(int P, int N, int M, const float* features_t, const float* t, double time, double period, float* shs, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_harmonic_features";
	if (const int rc = gsr_harmonic_inputs(who, P, N, M, features_t, t, period)) return rc;
	if (!shs) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: shs is NULL", who);
	gsr_launch_harmonic_forward(P, N, M, features_t, t, time, period, shs, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "harmonic_forward");
}

extern "C" int gsr_harmonic_features_backward(int P, int N, int M, const float* features_t, const float* t, double time, double period,
                                              const float* dL_dshs, float* dL_dfeatures_t, float* dL_dt, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_harmonic_features_backward";
	if (const int rc = gsr_harmonic_inputs(who, P, N, M, features_t, t, period)) return rc;
	if (!dL_dshs) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: dL_dshs is NULL", who);
	if (!dL_dfeatures_t && !dL_dt) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: both outputs are NULL", who);
	gsr_launch_harmonic_backward(P, N, M, features_t, t, time, period, dL_dshs, dL_dfeatures_t, dL_dt, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "harmonic_backward");
}

// ---- TSDF fusion and marching tetrahedra (include/gsr_tsdf.h) ----
// what every entry point refuses about the grid; 0 where there is nothing to refuse
static int gsr_tsdf_grid_check(const char* who, const gsr_tsdf_grid* g, int least)
{
	if (!g) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: grid is NULL", who);
	if (g->nx < least || g->ny < least || g->nz < least)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: every dimension must be at least %d (got %d x %d x %d)", who, least, g->nx, g->ny, g->nz);
	if ((long long)g->nx * g->ny > 0x7fffffffLL || (long long)g->nx * g->ny * g->nz > 0x7fffffffLL)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: %d x %d x %d nodes exceed 32-bit indexing", who, g->nx, g->ny, g->nz);
	if (!std::isfinite(g->origin[0]) || !std::isfinite(g->origin[1]) || !std::isfinite(g->origin[2]))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: the origin must be finite", who);
	if (!(g->voxel_size > 0.0f) || !std::isfinite(g->voxel_size))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: voxel_size must be finite and positive (got %g)", who, (double)g->voxel_size);
	return GSR_OK;
}

extern "C" int gsr_tsdf_integrate(const gsr_tsdf_grid* grid, float* wsum, float* dsum, float* csum, int C, const gsr_filter3d_camera* cameras,
                                  const gsr_filter3d_camera* cameras_host, int H, int W, const float* depth, const float* color, const float* weight,
                                  float sdf_trunc, float depth_trunc, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_tsdf_integrate";
	if (const int rc = gsr_tsdf_grid_check(who, grid, 1)) return rc;
	if (C < 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: C must be at least 1 (got %d)", who, C);
	if (H < 1 || W < 1 || H > (1 << 24) || W > (1 << 24) || (long long)H * W > 0x7fffffffLL)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: H and W must lie in 1 .. 2^24 with H W below 2^31 (got %d x %d)", who, H, W);
	if (!wsum || !dsum || !cameras || !depth) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: wsum, dsum, cameras or depth is NULL", who);
	if (color && !csum) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: color without csum", who);
	if (!(sdf_trunc > 0.0f) || !std::isfinite(sdf_trunc))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: sdf_trunc must be finite and positive (got %g)", who, (double)sdf_trunc);
	if (!(depth_trunc > 0.0f)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: depth_trunc must be positive or +inf (got %g)", who, (double)depth_trunc);
	if (cameras_host)
		for (int c = 0; c < C; c++)
			if (cameras_host[c].W != (float)W || cameras_host[c].H != (float)H)
				return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: camera %d is %g x %g, the depth maps are %d x %d", who, c, (double)cameras_host[c].W,
				                (double)cameras_host[c].H, W, H);
	gsr_launch_tsdf_integrate(*grid, wsum, dsum, csum, C, cameras, H, W, depth, color, weight, sdf_trunc, depth_trunc, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "tsdf_integrate");
}

extern "C" size_t gsr_tsdf_mesh_scratch_bytes(long long nodes)
{
	if (nodes < 8 || nodes > 0x7fffffffLL) return 0;
	return gsr_tsdf_mesh_scratch_size(nodes);
}

extern "C" int gsr_tsdf_mesh_plan(const gsr_tsdf_grid* grid, const float* wsum, const float* dsum, float min_weight, void* scratch,
                                  gsr_tsdf_mesh_plan_t* plan, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_tsdf_mesh_plan";
	if (plan) plan->magic = 0;
	if (const int rc = gsr_tsdf_grid_check(who, grid, 2)) return rc;
	if (!wsum || !dsum || !scratch || !plan) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: wsum, dsum, scratch or plan is NULL", who);
	if (((uintptr_t)scratch & 7) != 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: scratch must be 8-byte aligned", who);
	if (!(min_weight > 0.0f) || !std::isfinite(min_weight))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: min_weight must be finite and positive (got %g)", who, (double)min_weight);
	long long totals[2] = {0, 0};
	if (const int rc = gsr_check_hip(gsr_launch_tsdf_mesh_plan(*grid, wsum, dsum, min_weight, scratch, totals, (hipStream_t)stream), "tsdf_mesh_plan")) return rc;
	plan->V = totals[0]; plan->F = totals[1];
	plan->grid = *grid; plan->wsum = wsum; plan->dsum = dsum; plan->scratch = scratch; plan->min_weight = min_weight;
	plan->magic = GSR_TSDF_PLAN_MAGIC;
	return GSR_OK;
}

extern "C" int gsr_tsdf_mesh_emit(const gsr_tsdf_mesh_plan_t* plan, long long V, long long F, const float* csum, float* vertices, float* colors,
                                  int32_t* faces, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_tsdf_mesh_emit";
	if (!plan) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: plan is NULL", who);
	if (plan->magic != GSR_TSDF_PLAN_MAGIC) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: the plan was not filled in by gsr_tsdf_mesh_plan", who);
	if (const int rc = gsr_tsdf_grid_check(who, &plan->grid, 2)) return rc;
	if (!plan->wsum || !plan->dsum || !plan->scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: the plan holds a NULL pointer", who);
	if (V < 0 || F < 0 || V > 0x7fffffffLL || F > 0x7fffffffLL)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: V and F must lie in 0 .. 2^31 - 1 (got %lld, %lld)", who, V, F);
	if (V != plan->V || F != plan->F)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: V %lld, F %lld are not the plan's (%lld, %lld)", who, V, F, plan->V, plan->F);
	if (colors && !csum) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: colors without csum", who);
	if (V == 0) return GSR_OK;   // nothing to write
	if (!vertices || (F > 0 && !faces)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: vertices or faces is NULL", who);
	gsr_launch_tsdf_mesh_emit(*plan, csum, vertices, colors, faces, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "tsdf_mesh_emit");
}

extern "C" size_t gsr_knn_scratch_bytes(int P) { return gsr_knn_scratch_size(P); }

extern "C" int gsr_knn_mean_dist2(int P, const float* points, float* mean_dist2, void* scratch, void* stream)
{
	g_err[0] = 0;
	if (P < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_knn_mean_dist2: negative point count");
	if (P == 0) return GSR_OK;
	if (!points || !mean_dist2 || !scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_knn_mean_dist2: required pointer is NULL");
	if (!aligned16(scratch)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_knn_mean_dist2: scratch must be 16-byte aligned");
	gsr_launch_knn(P, points, mean_dist2, scratch, (hipStream_t)stream);
	return gsr_check_hip(hipGetLastError(), "knn kernels");
}

// ---- the neighbour graph (include/gsr_knn.h, knn_graph.hip) -----------------------------------------------
extern "C" size_t gsr_knn_search_scratch_bytes(int P, int Q) { return gsr_knn_search_scratch_size(P, Q); }

extern "C" int gsr_knn_search(int P, const float* points, int Q, const float* queries, int K, float* dist2, int* idx, void* scratch, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_knn_search";
	if (P < 0 || Q < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: negative count (P %d, Q %d)", who, P, Q);
	if (K < 1 || K > GSR_KNN_MAX_K) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: K must lie in 1..%d (got %d)", who, GSR_KNN_MAX_K, K);
	if (!queries && Q != P) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: the self-set form (queries NULL) needs Q == P (got %d, %d)", who, Q, P);
	if (P == 0 || Q == 0) return GSR_OK;
	if ((int64_t)Q * K > INT32_MAX) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: Q*K must stay below 2^31", who);
	if (!points || !dist2 || !idx || !scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: required pointer is NULL", who);
	if (!aligned16(scratch)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: scratch must be 16-byte aligned", who);
	gsr_launch_knn_search(P, points, Q, queries, K, dist2, idx, scratch, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "knn_search");
}

extern "C" size_t gsr_knn_graph_scratch_bytes(int E, int P) { return gsr_knn_graph_scratch_size(E, P); }

extern "C" int gsr_knn_graph_build(int E, const int* idx, int P, int* offsets, int* edges, int* num_valid, void* scratch, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_knn_graph_build";
	if (E < 0 || P < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: negative count (E %d, P %d)", who, E, P);
	if (P == INT32_MAX) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: P + 1 offsets must stay below 2^31", who);
	if (E == 0 || P == 0) {   // no edge has a target
		if (!offsets) return GSR_OK;
		gsr_launch_knn_graph_build(0, nullptr, P, offsets, nullptr, num_valid, nullptr, (hipStream_t)stream);
		return gsr_stage_done((hipStream_t)stream, 0, "knn_graph_build");
	}
	if (!idx || !offsets || !edges || !scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: required pointer is NULL", who);
	if (!aligned16(scratch)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: scratch must be 16-byte aligned", who);
	gsr_launch_knn_graph_build(E, idx, P, offsets, edges, num_valid, scratch, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "knn_graph_build");
}

extern "C" int gsr_knn_gather(int Q, int K, int C, const float* x, const int* idx, float* out, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_knn_gather";
	if (Q < 0 || K < 0 || C < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: negative count (Q %d, K %d, C %d)", who, Q, K, C);
	const int64_t E = (int64_t)Q * K;
	if (E > INT32_MAX || E * C >= ((int64_t)1 << 39)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: Q*K must stay below 2^31 and Q*K*C below 2^39", who);
	if (E == 0 || C == 0) return GSR_OK;
	if (!x || !idx || !out) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: required pointer is NULL", who);
	gsr_launch_knn_gather(E, C, x, idx, out, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "knn_gather");
}

extern "C" int gsr_knn_gather_backward(int P, int C, const int* offsets, const int* edges, const float* grad_out, float* grad_x, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_knn_gather_backward";
	if (P < 0 || C < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: negative count (P %d, C %d)", who, P, C);
	if ((int64_t)P * C >= ((int64_t)1 << 39)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: P*C must stay below 2^39", who);
	if (P == 0 || C == 0) return GSR_OK;
	if (!offsets || !edges || !grad_out || !grad_x) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: required pointer is NULL", who);
	gsr_launch_knn_gather_backward(P, C, offsets, edges, grad_out, grad_x, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "knn_gather_bwd");
}

// ---- vector quantisation (include/gsr_vq.h, vq.hip) -----------------------------------------------------------
static int gsr_vq_check(const char* who, int N, int D, int K)
{
	if (N < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: negative count (N %d)", who, N);
	if (D < 1 || D > GSR_VQ_MAX_D) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: D must lie in 1..%d (got %d)", who, GSR_VQ_MAX_D, D);
	if (K < 1 || K > GSR_VQ_MAX_K) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: K must lie in 1..%d (got %d)", who, GSR_VQ_MAX_K, K);
	return GSR_OK;
}

extern "C" size_t gsr_vq_assign_scratch_bytes(int N, int D, int K) { return gsr_vq_assign_scratch_size(N, D, K); }

extern "C" int gsr_vq_assign(int N, int D, const float* x, int K, const float* codebook, int* idx, float* dist2, void* scratch, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_vq_assign";
	if (const int rc = gsr_vq_check(who, N, D, K)) return rc;
	if (N == 0) return GSR_OK;
	if (!x || !codebook || !idx || !scratch) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: required pointer is NULL", who);
	if (!aligned16(scratch)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: scratch must be 16-byte aligned", who);
	gsr_launch_vq_assign(N, D, x, K, codebook, idx, dist2, scratch, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "vq_assign");
}

extern "C" int gsr_vq_update(int N, int D, const float* x, const float* weight, int K, const int* offsets, const int* members, float* codebook,
                             int* count, float* wsum, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_vq_update";
	if (const int rc = gsr_vq_check(who, N, D, K)) return rc;
	if (N == 0) return GSR_OK;
	if (!x || !offsets || !members || !codebook) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: required pointer is NULL", who);
	gsr_launch_vq_update(D, x, weight, K, offsets, members, codebook, count, wsum, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "vq_update");
}

// ---- the neighbour-rigidity losses (include/gsr_rigidity.h, rigidity.hip) ------------------------------------
static bool gsr_rigidity_fits(int P, int K) { return P >= 0 && K >= 0 && K <= GSR_RIGIDITY_MAX_K && (int64_t)P * K <= INT32_MAX; }

extern "C" size_t gsr_rigidity_scratch_bytes(int P, int K) { return gsr_rigidity_fits(P, K) ? gsr_rigidity_scratch_size(P, K) : 0; }

extern "C" int gsr_rigidity_loss(int P, int K, const float* xyz, const float* rotation, const int* idx, const float* prev_offset, const float* prev_dist,
                                 const float* weight, const float* prev_inv_rot, const int* offsets, const int* edges, float w_rigid, float w_rot,
                                 float w_iso, float* values, float* grad_xyz, float* grad_rot, void* scratch, void* stream)
{
	g_err[0] = 0;
	const char* who = "gsr_rigidity_loss";
	if (P < 0 || K < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: negative count (P %d, K %d)", who, P, K);
	if (K > GSR_RIGIDITY_MAX_K) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: K must lie in 1..%d (got %d)", who, GSR_RIGIDITY_MAX_K, K);
	if (!values) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: values is NULL", who);
	if ((int64_t)P * K > INT32_MAX) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: P*K must stay below 2^31", who);
	if (P == 0 || K == 0) {   // no edge: zeros
		gsr_launch_rigidity_zero(P, values, grad_xyz, grad_rot, (hipStream_t)stream);
		return gsr_stage_done((hipStream_t)stream, 0, "rigidity_fold");
	}
	if (!xyz || !rotation || !idx || !prev_offset || !prev_dist || !weight || !prev_inv_rot || !offsets || !scratch)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: required pointer is NULL", who);
	if ((grad_xyz || grad_rot) && !edges) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: edges is NULL and a gradient is asked for", who);
	if (!aligned16(scratch)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: scratch must be 16-byte aligned", who);
	gsr_launch_rigidity_loss(P, K, xyz, rotation, idx, prev_offset, prev_dist, weight, prev_inv_rot, offsets, edges, w_rigid, w_rot, w_iso, values, grad_xyz,
	                         grad_rot, scratch, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "rigidity_fold");
}

extern "C" int gsr_adam_step(int ngroups, const gsr_adam_group* groups, double beta1, double beta2, double eps,
                             const int* radii, void* stream)
{
	g_err[0] = 0;
	if (ngroups < 0 || ngroups > GSR_ADAM_MAX_GROUPS) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_adam_step: 0..%d groups", GSR_ADAM_MAX_GROUPS);
	if (ngroups == 0) return GSR_OK;
	if (!groups) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_adam_step: groups is NULL");
	for (int k = 0; k < ngroups; k++) {
		const gsr_adam_group& g = groups[k];
		if (g.numel < 0 || g.step < 1 || (g.numel > 0 && (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq)))
			return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_adam_step: group %d: NULL tensor, negative size or step < 1", k);
		if (g.numel > ((int64_t)1 << 41)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_adam_step: group %d too large", k);
		if (radii && (g.row <= 0 || g.numel % g.row != 0))
			return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_adam_step: group %d: numel is not a multiple of row", k);
	}
	int64_t total = 0;
	for (int k = 0; k < ngroups; k++) total += groups[k].numel;
	if (total == 0) return GSR_OK;  // nothing to launch
	hipStream_t s = (hipStream_t)stream;
	{
		GsrProfScope p(s, "adam");
		gsr_launch_adam(ngroups, groups, beta1, beta2, eps, radii, s);
	}
	return gsr_check_hip(hipGetLastError(), "gsr_adam_kernel launch");
}

extern "C" int gsr_sh_grad_from_views(int P, int D, int M, int V, const float* means3D, const float* cam_pos,
                                      const float* dL_dRGB, int64_t view_stride, float* dL_dsh, void* stream)
{
	g_err[0] = 0;
	if (P < 0 || V < 0 || D < 0 || D > 3 || M <= 0 || M > 16 || (D + 1) * (D + 1) > M)
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_sh_grad_from_views: bad sizes (P %d, V %d, D %d, M %d)", P, V, D, M);
	if (P == 0) return GSR_OK;
	if (!means3D || !dL_dsh || (V > 0 && (!cam_pos || !dL_dRGB)))
		return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_sh_grad_from_views: NULL pointer");
	if (view_stride == 0) view_stride = (int64_t)P * 3;
	if (view_stride < (int64_t)P * 3) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_sh_grad_from_views: view_stride < 3 * P");
	gsr_launch_sh_grad_from_views(P, D, M, V, means3D, cam_pos, dL_dRGB, view_stride, dL_dsh, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "sh_grad_from_views");
}

extern "C" int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                                uint8_t* present, void* stream)
{
	g_err[0] = 0;
	(void)projmatrix;
	if (P < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "bad P");
	if (P == 0) return GSR_OK;
	if (!means3D || !viewmatrix || !present) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mark_visible: NULL pointer");
	gsr_launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream);
	return gsr_stage_done((hipStream_t)stream, 0, "mark_visible");
}
