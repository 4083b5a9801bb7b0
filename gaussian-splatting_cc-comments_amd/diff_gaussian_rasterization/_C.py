"""ctypes binding of libgsr_hip.so with the surface of the reference's torch extension
`diff_gaussian_rasterization._C` (submodules/diff-gaussian-rasterization/ext.cpp:18-22):

    rasterize_gaussians(...)          -> rasterize_points.cu:38-130  RasterizeGaussiansCUDA
    rasterize_gaussians_backward(...) -> rasterize_points.cu:132-216 RasterizeGaussiansBackwardCUDA
    mark_visible(...)                 -> rasterize_points.cu:218-237 markVisible

Same positional arguments, same return tuples.  PyTorch is only the allocator and the stream
provider here: every tensor is handed to the C ABI (include/gsr.h) as a raw device pointer.
There is no CPU fallback: a missing library or a non-HIP tensor raises.
"""
import ctypes
import math
import os
from typing import NamedTuple, Optional

import torch

from . import _binding

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(os.path.dirname(_HERE), "libgsr_hip.so")   # nothing in the environment changes this: see use_library()
_lib = None

_vp = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64
_f = ctypes.c_float
_sz = ctypes.c_size_t


class GeometryLayout(ctypes.Structure):
    _fields_ = [(n, _sz) for n in ("splat", "depth_keys", "depth_keys_alt", "perm", "perm_alt", "tiles_touched", "rect",
                                   "slot_base", "clamped", "sh_ddir", "status", "scan_temp", "sort_table", "col_table", "rshape", "total")]


class ImageLayout(ctypes.Structure):
    _fields_ = [(n, _sz) for n in ("final_C", "final_T", "n_contrib", "ranges", "tile_max_contrib", "tile_order", "total")]


class BinningLayout(ctypes.Structure):
    _fields_ = [(n, _sz) for n in ("point_list", "point_list_alt", "tile_keys", "tile_keys_alt", "sort_table",
                                   "checkpoints", "total", "tile_key_bytes", "column_pairs", "band_masks")]


class KernelTime(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("ms", _f)]


class BackwardArgs(ctypes.Structure):
    """include/gsr.h gsr_backward_args (the two-stage backward: gsr_backward_blend / gsr_backward_gaussians)"""
    _fields_ = ([("P", _i), ("D", _i), ("M", _i), ("num_rendered", _i64), ("width", _i), ("height", _i), ("leaf", _i)] +
                [(n, _vp) for n in ("background", "means3D", "shs", "shs_rest", "colors_precomp", "scales")] +
                [("scale_modifier", _f)] +
                [(n, _vp) for n in ("rotations", "cov3D_precomp", "viewmatrix", "projmatrix", "cam_pos")] +
                [("tan_fovx", _f), ("tan_fovy", _f)] +
                [(n, _vp) for n in ("radii", "geometry", "binning", "image", "scratch", "dL_dpix", "dL_dmean2D", "dL_dconic",
                                    "dL_dopacity", "dL_dcolor", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dsh_rest", "dL_dscale",
                                    "dL_drot", "stat_xyz_gradient_accum", "stat_denom", "stat_max_radii2D", "stream")] +
                [("debug", _i)])


AUX_MODES = {"depth": 1, "invdepth": 2}   # GSR_AUX_DEPTH / GSR_AUX_INVDEPTH


class AuxArgs(ctypes.Structure):
    """include/gsr_aux.h gsr_aux_args (the depth and alpha maps; opt-in, kernels of their own)"""
    _fields_ = [("mode", _i), ("out_depth", _vp), ("out_alpha", _vp), ("dL_ddepth", _vp), ("dL_dalpha", _vp), ("scratch", _vp)]


class CamArgs(ctypes.Structure):
    """include/gsr_cam.h gsr_cam_args"""
    _fields_ = [("dL_dviewmatrix", _vp), ("dL_dprojmatrix", _vp), ("dL_dcampos", _vp), ("scratch", _vp)]


class CamCmArgs(ctypes.Structure):
    """include/gsr_cam_cm.h gsr_cam_cm_args"""
    _fields_ = [("dL_dviewmatrix", _vp), ("dL_dintrinsics", _vp), ("dL_dcampos", _vp), ("scratch", _vp)]


class AbsgradArgs(ctypes.Structure):
    """include/gsr_absgrad.h gsr_absgrad_args"""
    _fields_ = [("abs_dL_dmean2D", _vp), ("stat_abs_gradient_accum", _vp)]


class CameraModelArgs(ctypes.Structure):
    """include/gsr_camera_model.h gsr_camera_model"""
    _fields_ = [("model", _i), ("fx", _f), ("fy", _f), ("cx", _f), ("cy", _f)]


CAMERA_MODELS = {"pinhole": 0, "fisheye": 1}   # GSR_CAMERA_PINHOLE / GSR_CAMERA_FISHEYE


class CameraModel(NamedTuple):
    """A camera model of include/gsr_camera_model.h: model "pinhole" (with intrinsics: an off-centre principal point) or "fisheye"
    (equidistant, no distortion coefficients); fx, fy in pixels; cx, cy in pixels in the OpenCV / COLMAP convention (origin at the
    corner of the first pixel, pixel centres at +0.5).  The default camera of a W x H image is
    CameraModel("pinhole", W / (2 tanfovx), H / (2 tanfovy), W / 2, H / 2)."""
    model: str
    fx: float
    fy: float
    cx: float
    cy: float

    @classmethod
    def from_tensor(cls, model, intrinsics):
        """The CameraModel whose floats are the values of `intrinsics`, a (4,) tensor (fx, fy, cx, cy) -- the tensor that
        `camera_model_grads=` takes as the autograd handle of the intrinsics.  One read-back from the device: the kernels take the
        model's floats as arguments, so an optimiser step on the tensor is followed by this call."""
        if not isinstance(intrinsics, torch.Tensor) or tuple(intrinsics.shape) != (4,):
            raise ValueError(f"intrinsics must be a tensor of shape (4,) holding (fx, fy, cx, cy), got {intrinsics!r}")
        return camera_model((model, *(float(v) for v in intrinsics.detach().to(torch.float32).cpu().tolist())))


class AuxLayout(ctypes.Structure):
    _fields_ = [(n, _sz) for n in ("ckpt_depth", "final_D", "total")]


# bits of the C ABI's `debug` mask (include/gsr.h GSR_DEBUG_*).  The reference's bool `debug` is DEBUG_SYNC; tests pass the
# diagnostic bits as an int in the same argument, per call -- nothing is read from the environment.
DEBUG_SYNC, DEBUG_NO_CULL, DEBUG_SERIAL, DEBUG_NO_SPLIT, DEBUG_TILE_SORT, DEBUG_RADIX_DEPTH, DEBUG_NO_TRIM = 1, 2, 4, 8, 16, 32, 64
DEBUG_MEDIAN_FULL_WALK = 128   # include/gsr_median.h: median_forward() without its early exit
DEBUG_RECOMPUTE_BANDS = 256    # the backward blend computes the band masks itself instead of reading the forward's bytes


def _dbg(debug):
    return int(debug) if (isinstance(debug, int) and not isinstance(debug, bool)) else int(bool(debug))


# ---- the entry points this module calls, header by header (_binding.declare; tests/test_binding_cpu.py holds them to include/*.h) ----
_str, _u32, _dbl, _pi64 = ctypes.c_char_p, ctypes.c_uint32, ctypes.c_double, ctypes.POINTER(_i64)
_pa, _pb, _pm = ctypes.POINTER(AuxArgs), ctypes.POINTER(BackwardArgs), ctypes.POINTER(CameraModelArgs)
_PRE = [_i] * 5 + [_vp] * 5 + [_f] + [_vp] * 5 + [_f, _f, _i, _vp, _vp, _pi64, _vp, _i]        # gsr_forward_preprocess
_PRE_LEAF = [_i] * 5 + [_vp] * 5 + [_f] + [_vp] * 4 + [_f, _f, _i, _vp, _vp, _pi64, _vp, _i]   # gsr_forward_preprocess_leaf
_RENDER = [_i, _i64, _i, _i] + [_vp] * 7 + [_i]                                               # gsr_forward_render
_STATE = [_i, _i64, _i, _i] + [_vp] * 3    # the sizes and the three state buffers in front of a replay pass's own arguments
_binding.declare("gsr.h", {
    "gsr_last_error": (_str, []), "gsr_version": (_str, []), "gsr_thread_release": (_i, []),
    "gsr_geometry_bytes": (_sz, [_i]), "gsr_image_bytes": (_sz, [_i, _i]), "gsr_binning_bytes": (_sz, [_i, _i64, _i, _i]),
    "gsr_backward_scratch_bytes": (_sz, [_i, _i64]),
    "gsr_geometry_layout_of": (_i, [_i, ctypes.POINTER(GeometryLayout)]),
    "gsr_image_layout_of": (_i, [_i, _i, ctypes.POINTER(ImageLayout)]),
    "gsr_binning_layout_of": (_i, [_i, _i64, _i, _i, ctypes.POINTER(BinningLayout)]),
    "gsr_get_higher_msb": (_u32, [_u32]),
    "gsr_forward_preprocess": (_i, _PRE), "gsr_forward_render": (_i, _RENDER),
    "gsr_backward": (_i, [_i, _i, _i, _i64, _i, _i] + [_vp] * 5 + [_f] + [_vp] * 5 + [_f, _f] + [_vp] * 16 + [_i]),
    "gsr_backward_blend": (_i, [_pb]), "gsr_backward_gaussians": (_i, [_pb, _i, _i, _i]),
    "gsr_mark_visible": (_i, [_i] + [_vp] * 5),
    "gsr_sh_grad_from_views": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _i64, _vp, _vp]),
    "gsr_profile_begin": (_i, [_vp]), "gsr_profile_begin_only": (_i, [_vp, _str]),
    "gsr_profile_end": (_i, [_vp, ctypes.POINTER(KernelTime), _i]),
    # the leaf-parameter forward (fused_params.py), its one-call backward (bound, not called: the two stages serve every variant) and
    # the optimiser step (its groups: fused_params.AdamGroup)
    "gsr_forward_preprocess_leaf": (_i, _PRE_LEAF),
    "gsr_backward_leaf": (_i, [_i, _i, _i, _i64, _i, _i] + [_vp] * 5 + [_f] + [_vp] * 4 + [_f, _f] + [_vp] * 15 + [_i]),
    "gsr_adam_step": (_i, [_i, _vp, _dbl, _dbl, _dbl, _vp, _vp]),
}, {"gsr_geometry_layout": GeometryLayout, "gsr_image_layout": ImageLayout, "gsr_binning_layout": BinningLayout,
    "gsr_kernel_time": KernelTime, "gsr_backward_args": BackwardArgs})
# depth and alpha maps, the screen-space filter, a camera model: the same calls with leading arguments
_binding.declare("gsr_aux.h", {
    "gsr_aux_bytes": (_sz, [_i64, _i, _i]), "gsr_aux_layout_of": (_i, [_i64, _i, _i, ctypes.POINTER(AuxLayout)]),
    "gsr_forward_preprocess_aux": (_i, [_pa] + _PRE), "gsr_forward_preprocess_leaf_aux": (_i, [_pa] + _PRE_LEAF),
    "gsr_forward_render_aux": (_i, [_pa] + _RENDER),
    "gsr_backward_blend_aux": (_i, [_pb, _pa]), "gsr_backward_gaussians_aux": (_i, [_pb, _pa, _i, _i, _i]),
}, {"gsr_aux_args": AuxArgs, "gsr_aux_layout": AuxLayout})
_binding.declare("gsr_aa.h", {
    "gsr_forward_preprocess_aa": (_i, [_i, _pa] + _PRE), "gsr_forward_preprocess_leaf_aa": (_i, [_i, _pa] + _PRE_LEAF),
    "gsr_backward_gaussians_aa": (_i, [_pb, _i, _vp, _pa, _i, _i, _i]),
})
_binding.declare("gsr_camera_model.h", {
    "gsr_forward_preprocess_cm": (_i, [_pm, _i, _pa] + _PRE), "gsr_forward_preprocess_leaf_cm": (_i, [_pm, _i, _pa] + _PRE_LEAF),
    "gsr_backward_gaussians_cm": (_i, [_pb, _pm, _i, _vp, _pa, _i, _i, _i]),
}, {"gsr_camera_model": CameraModelArgs})
_binding.declare("gsr_cam.h", {
    "gsr_cam_bytes": (_sz, [_i]),
    "gsr_backward_gaussians_cam": (_i, [_pb, _i, _vp, _pa, ctypes.POINTER(CamArgs), _i, _i, _i]),
}, {"gsr_cam_args": CamArgs})
_binding.declare("gsr_cam_cm.h", {
    "gsr_cam_cm_bytes": (_sz, [_i]),
    "gsr_backward_gaussians_cam_cm": (_i, [_pb, _pm, _i, _vp, _pa, ctypes.POINTER(CamCmArgs), _i, _i, _i]),
}, {"gsr_cam_cm_args": CamCmArgs})
_binding.declare("gsr_absgrad.h", {
    "gsr_backward_blend_abs": (_i, [_pb, _pa, _i]), "gsr_absgrad_fold": (_i, [_pb, ctypes.POINTER(AbsgradArgs), _i, _i]),
}, {"gsr_absgrad_args": AbsgradArgs})
# passes that replay the forward's state: blend-weight statistics, feature channels, the distortion and median-depth maps
_binding.declare("gsr_contrib.h", {
    "gsr_contrib_scratch_bytes": (_sz, [_i, _i64]), "gsr_contributions": (_i, _STATE + [_vp] * 6 + [_i]),
})
_binding.declare("gsr_features.h", {
    "gsr_features_scratch_bytes": (_sz, [_i, _i64, _i]),
    "gsr_features_forward": (_i, [_i, _i64, _i, _i, _i] + [_vp] * 6 + [_i]),
    "gsr_features_backward": (_i, [_pb, _i, _vp, _vp, _vp, _vp, _i]),
})
_binding.declare("gsr_distortion.h", {
    "gsr_distortion_state_bytes": (_sz, [_i, _i]), "gsr_distortion_forward": (_i, _STATE + [_vp] * 3 + [_i]),
    "gsr_distortion_backward": (_i, [_pb, _vp, _vp]),
})
_binding.declare("gsr_median.h", {
    "gsr_median_state_bytes": (_sz, [_i, _i]), "gsr_median_forward": (_i, _STATE + [_vp] * 6 + [_i]),
    "gsr_median_backward": (_i, [_pb, _vp, _vp]),
})
# per-Gaussian normals, depth normals and the normal-consistency loss (fused_geometry.py)
_binding.declare("gsr_normals.h", {
    "gsr_gaussian_normals": (_i, [_i] + [_vp] * 4 + [_i, _vp, _vp]),
    "gsr_gaussian_normals_backward": (_i, [_i] + [_vp] * 4 + [_i, _vp, _vp, _vp]),
    "gsr_normals_scratch_bytes": (_sz, [_i, _i]),
    "gsr_depth_normals": (_i, [_i, _i, _vp, _f, _f, _vp, _vp]),
    "gsr_depth_normals_backward": (_i, [_i, _i, _vp, _f, _f, _vp, _vp, _vp]),
    "gsr_normal_consistency_loss": (_i, [_i, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp]),
})


def library_path():
    return _LIB_PATH


def use_library(path):
    """Diagnostics (tools/tile_clock.py, bench.py --library): bind another build of the same C ABI -- the per-tile-clock twin, an
    A/B variant of one translation unit -- instead of the product library.  Must be called before the first lib(); the product
    never calls it."""
    global _LIB_PATH
    if _lib is not None:
        raise RuntimeError("use_library() must be called before the library is first loaded")
    _LIB_PATH = os.path.abspath(path)


def lib():
    """Load libgsr_hip.so (once).  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"{_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the rasterizer.")
    _lib = _binding.bind(ctypes.CDLL(_LIB_PATH))
    return _lib


_aux_lib = _aa_lib = lib   # every entry point is declared by lib()
_check = _binding.check    # the status of an entry point: anything but 0 raises with the library's message


def _ptr(t):
    """Raw device pointer; an empty tensor is the reference's "not provided" and becomes NULL
    (rasterize_points.cu:108-125)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def _dev_f32(t, device, what):
    if t.numel() == 0:
        return t
    if t.device != device:
        raise RuntimeError(f"{what} must be on {device} (got {t.device}); the HIP rasterizer has no CPU path")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what} must be float32 (got {t.dtype})")
    return t.contiguous()


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def aux_mode(name):
    """"depth" / "invdepth" -> the C ABI's mode; anything else raises ValueError."""
    if not isinstance(name, str) or name not in AUX_MODES:
        raise ValueError(f"depth_alpha must be one of {sorted(AUX_MODES)} or None, got {name!r}")
    return AUX_MODES[name]


def aa_flag(antialiasing):
    """The `antialiasing` keyword -> bool; anything but a bool raises TypeError (a mode string or a number is not a switch here)."""
    if not isinstance(antialiasing, bool):
        raise TypeError(f"antialiasing must be True or False, got {antialiasing!r}")
    return antialiasing


def camera_flag(camera_grads):
    """The `camera_grads` keyword -> bool; anything but a bool raises TypeError, like `antialiasing`."""
    if not isinstance(camera_grads, bool):
        raise TypeError(f"camera_grads must be True or False, got {camera_grads!r}")
    return camera_grads


def camera_model(cm):
    """Checks the `camera_model` keyword: None, a CameraModel or any 5-tuple (model, fx, fy, cx, cy) -> None or a CameraModel of
    Python floats.  Anything else raises TypeError (numbers that are no real numbers too); a model string other than "pinhole" /
    "fisheye", a focal length that is not finite and positive and a principal point that is not finite raise ValueError.  No
    library is touched."""
    if cm is None:
        return None
    if not isinstance(cm, tuple) or len(cm) != 5:
        raise TypeError(f"camera_model must be a CameraModel or a 5-tuple (model, fx, fy, cx, cy), got {cm!r}")
    model, *nums = cm
    if not isinstance(model, str):
        raise TypeError(f"camera_model: model must be a string, got {model!r}")
    if model not in CAMERA_MODELS:
        raise ValueError(f"camera_model: model must be one of {sorted(CAMERA_MODELS)}, got {model!r}")
    if any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in nums):
        raise TypeError(f"camera_model: fx, fy, cx, cy must be real numbers, got {tuple(nums)!r}")
    fx, fy, cx, cy = (float(v) for v in nums)
    if not (math.isfinite(fx) and math.isfinite(fy) and fx > 0.0 and fy > 0.0):
        raise ValueError(f"camera_model: fx and fy must be finite and positive, got {fx}, {fy}")
    if not (math.isfinite(cx) and math.isfinite(cy)):
        raise ValueError(f"camera_model: cx and cy must be finite, got {cx}, {cy}")
    return CameraModel(model, fx, fy, cx, cy)


def camera_model_args(cm):
    """A checked CameraModel (camera_model()) or None -> CameraModelArgs or None"""
    if cm is None:
        return None
    return CameraModelArgs(CAMERA_MODELS[cm.model], cm.fx, cm.fy, cm.cx, cm.cy)


def camera_model_excludes(cm, camera_grads=False, what=None):
    """The combinations a camera model has no form for, refused with NotImplementedError before anything runs: the camera gradients
    (their 27 terms differentiate projmatrix), and `what`, the name of a path without one."""
    if cm is None:
        return
    if what is not None:
        raise NotImplementedError(f"{what} has no camera_model form")
    if camera_grads is True:
        raise NotImplementedError("camera_grads=True has no camera_model form: the camera gradients differentiate projmatrix, "
                                  "which a camera model ignores; camera_model_grads=True gives dL/dviewmatrix, dL/dcampos and "
                                  "dL/dintrinsics under a model")


def camera_model_grads_arg(value, cm, device=None):
    """Checks the `camera_model_grads` keyword against the checked CameraModel `cm` (or None) -> False, True, or the intrinsics tensor.
    False: nothing.  True: the settings' viewmatrix and campos become autograd inputs behind the model (include/gsr_cam_cm.h).  A
    float32 (4,) HIP tensor: as True, and the tensor is the autograd handle of (fx, fy, cx, cy): it receives dL/dintrinsics; its
    values are not read (CameraModel.from_tensor builds the model from it).  Anything but a bool or a tensor raises TypeError; a
    wrong dtype, shape or device, and True or a tensor without a camera model, ValueError.  No library is touched."""
    if isinstance(value, bool):
        if value and cm is None:
            raise ValueError("camera_model_grads=True needs a camera_model (without one, camera_grads=True gives dL/dviewmatrix, "
                             "dL/dprojmatrix and dL/dcampos)")
        return value
    if not isinstance(value, torch.Tensor):
        raise TypeError(f"camera_model_grads must be True, False or a float32 (4,) tensor (fx, fy, cx, cy), got {value!r}")
    if cm is None:
        raise ValueError("camera_model_grads needs a camera_model: the tensor is the autograd handle of that model's intrinsics")
    if value.dtype != torch.float32:
        raise ValueError(f"camera_model_grads: the intrinsics tensor must be float32 (got {value.dtype})")
    if tuple(value.shape) != (4,):
        raise ValueError(f"camera_model_grads: the intrinsics tensor must have shape (4,) = (fx, fy, cx, cy), got {tuple(value.shape)}")
    if not value.is_cuda or (device is not None and value.device != device):
        raise ValueError(f"camera_model_grads: the intrinsics tensor must be on the render's HIP (cuda) device (got {value.device})")
    return value


def camera_model_matches(cm, intrinsics):
    """settings.debug: the intrinsics tensor of `camera_model_grads` and the CameraModel the kernels read must hold the same float32
    values (one read-back); ValueError otherwise."""
    want = torch.tensor([cm.fx, cm.fy, cm.cx, cm.cy], dtype=torch.float32)
    got = intrinsics.detach().to(torch.float32).cpu()
    if not torch.equal(want, got):
        raise ValueError(f"camera_model_grads: the intrinsics tensor {got.tolist()} differs from the camera_model's "
                         f"(fx, fy, cx, cy) = {want.tolist()}; build the model with CameraModel.from_tensor(model, intrinsics)")


def absgrad_tensors(absgrad, P, device=None):
    """Checks the `absgrad` keyword: (abs_mean2D float32 [P, 2] or None, abs_gradient_accum float32 [P] or None), contiguous tensors
    on `device` (None: any HIP device, the same for both) -> AbsgradArgs.  Anything but a 2-tuple raises TypeError; a wrong dtype,
    shape or device, a non-contiguous tensor and two Nones raise ValueError.  No kernel and no library is touched."""
    if not isinstance(absgrad, (tuple, list)) or len(absgrad) != 2:
        raise TypeError(f"absgrad must be a 2-tuple (abs_mean2D, abs_gradient_accum), got {absgrad!r}")
    if any(t is not None and not isinstance(t, torch.Tensor) for t in absgrad):
        raise TypeError("absgrad must hold tensors or None")
    if all(t is None for t in absgrad):
        raise ValueError("absgrad must hold at least one tensor: (abs_mean2D, abs_gradient_accum) are both None")
    c = AbsgradArgs()
    for field, name, t, shape in zip(("abs_dL_dmean2D", "stat_abs_gradient_accum"), ("abs_mean2D", "abs_gradient_accum"), absgrad,
                                     ((int(P), 2), (int(P),))):
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32 (got {t.dtype})")
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32 tensor of shape {shape} (got shape {tuple(t.shape)}, "
                             f"{'' if t.is_contiguous() else 'not '}contiguous)")
        if not t.is_cuda:
            raise ValueError(f"{name} must be a HIP (cuda) tensor (got {t.device}); the HIP rasterizer has no CPU path")
        device = t.device if device is None else device
        if t.device != device:
            raise ValueError(f"{name} must be on {device} (got {t.device})")
        setattr(c, field, _ptr(t))
    c._keep = tuple(absgrad)
    return c


# which camera inputs take part in autograd (RenderOptions.camera) -> the inputs whose gradients the backward's camera target holds,
# in the order of its struct: gsr_cam_args (include/gsr_cam.h) / gsr_cam_cm_args (include/gsr_cam_cm.h)
CAMERA_TARGETS = {"cam": ("viewmatrix", "projmatrix", "campos"), "cm": ("viewmatrix", "intrinsics", "campos")}
_CAMERA_SHAPES = {"viewmatrix": (4, 4), "projmatrix": (4, 4), "campos": (3,), "intrinsics": (4,)}


def camera_target(kind, P, device):
    """The camera target of a backward, kind "cam" or "cm" -> (CamArgs / CamCmArgs, the three gradients of CAMERA_TARGETS[kind]):
    the outputs, which the fold kernel writes in full, and the scratch of P Gaussians, all from torch's allocator; the struct keeps
    them alive until the calls that use it have been enqueued.  P == 0, where nothing is launched: (None, zeros)."""
    f32 = dict(dtype=torch.float32, device=device)
    shapes = [_CAMERA_SHAPES[n] for n in CAMERA_TARGETS[kind]]
    if P == 0:
        return None, tuple(torch.zeros(s, **f32) for s in shapes)
    outs = tuple(torch.empty(s, **f32) for s in shapes)
    nbytes = lib().gsr_cam_bytes(int(P)) if kind == "cam" else lib().gsr_cam_cm_bytes(int(P))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=device)
    c = CamArgs() if kind == "cam" else CamCmArgs()
    for (field, _), t in zip(c._fields_, outs + (scratch,)):
        setattr(c, field, t.data_ptr())
    c._keep = outs + (scratch,)
    return c, outs


class RenderOptions(NamedTuple):
    """Everything of one render that is no differentiable input, checked: the one record the public entry points hand to the autograd
    Functions (render_options() builds it).  camera: which camera inputs take part in autograd -- None, "cam" (the settings'
    viewmatrix, projmatrix and campos, include/gsr_cam.h) or "cm" (viewmatrix, campos and the intrinsics tensor under camera_model,
    include/gsr_cam_cm.h); the tied inputs are CAMERA_TARGETS[camera]."""
    depth_alpha: Optional[str] = None
    antialiasing: bool = False
    densify_stats: Optional[tuple] = None
    contrib_stats: Optional[tuple] = None
    contrib_pixel_weight: Optional[torch.Tensor] = None
    absgrad: Optional[tuple] = None
    distortion: bool = False
    median_depth: bool = False
    index_maps: Optional[tuple] = None
    camera_model: Optional[CameraModel] = None
    camera: Optional[str] = None


def render_options(raster_settings, depth_alpha=None, densify_stats=None, antialiasing=False, contrib_stats=None,
                   contrib_pixel_weight=None, camera_grads=False, absgrad=None, distortion=False, median_depth=False, index_maps=None,
                   model=None, camera_model_grads=False, mode_required=False):
    """The public keywords -> (RenderOptions, the intrinsics tensor of camera_model_grads or None).  Runs every check that needs
    neither P nor a device, in one order for every entry point: depth_alpha (ValueError), distortion and median_depth (TypeError for
    anything but a bool, ValueError without a mode), index_maps (TypeError / ValueError), antialiasing and camera_grads (TypeError),
    model, the `camera_model` keyword (TypeError / ValueError; NotImplementedError with camera_grads), camera_model_grads (TypeError /
    ValueError).
    mode_required: depth_alpha=None is refused too (rasterize_gaussians_depth_alpha)."""
    if depth_alpha is not None or mode_required:
        aux_mode(depth_alpha)
    distortion_flag(distortion, depth_alpha)
    median_flag(median_depth, depth_alpha)
    if index_maps is not None:
        index_map_tensors(index_maps, raster_settings.image_width, raster_settings.image_height)
    aa_flag(antialiasing)
    camera_flag(camera_grads)
    cm = camera_model(model)
    camera_model_excludes(cm, camera_grads)
    cmg = camera_model_grads_arg(camera_model_grads, cm)
    camera = "cm" if cmg is not False else "cam" if camera_grads else None
    return (RenderOptions(depth_alpha, antialiasing, densify_stats, contrib_stats, contrib_pixel_weight, absgrad, distortion,
                          median_depth, index_maps, cm, camera), cmg if isinstance(cmg, torch.Tensor) else None)


def check_render_tensors(options, features, intrinsics, P, device, raster_settings):
    """The checks of a render's options that need P and the render's device (None: the render is not on a HIP device and will be
    refused by the forward itself), at the top of every autograd forward: refused before anything runs.  A record that did not come
    from render_options() is held to its rule for the maps too.  With settings.debug the intrinsics tensor and the model must agree."""
    distortion_flag(options.distortion, options.depth_alpha)
    median_flag(options.median_depth, options.depth_alpha)
    if options.index_maps is not None:
        index_map_tensors(options.index_maps, raster_settings.image_width, raster_settings.image_height, device)
    if features is not None:
        feature_tensor(features, P, device)
    if options.contrib_stats is not None:
        contrib_stat_tensors(options.contrib_stats, P)
    if options.absgrad is not None:   # only the backward writes the tensors
        absgrad_tensors(options.absgrad, P, device)
    if intrinsics is not None and raster_settings.debug:
        camera_model_matches(options.camera_model, intrinsics)


# ---- which C entry point serves a variant: the only place that chooses between gsr_*, gsr_*_aux and gsr_*_aa -------------------
def _entry(L, stage, leaf=False, x=None, aa=False, opacities=None, cam=None, absgrad=False, cm=None):
    """-> (function of L, the arguments that precede the default entry point's own).  stage: "preprocess" | "render" (the two forward
    calls) | "blend" | "gaussians" (the two backward stages: their leading arguments follow the gsr_backward_args pointer); leaf: the
    inputs are the optimiser's leaves (fused_params.py); x: the AuxArgs of a call with depth and alpha maps, or None; aa: the
    screen-space filter, whose per-Gaussian backward reads the forward's opacity input at address `opacities`.  The *_aa entry
    points take (antialiasing, aux or NULL, ...) and cover every other one; the older names stay in use where they suffice.
    cam: the CamArgs of a per-Gaussian backward that also produces the camera gradients (include/gsr_cam.h), or None; with cm, the
    CamCmArgs of the camera gradients under that model (include/gsr_cam_cm.h).
    absgrad: the blend that also leaves the sums of per-pixel moduli in the slots (include/gsr_absgrad.h).
    cm: the CameraModelArgs of a call with a camera model (include/gsr_camera_model.h), or None: the *_cm entry points take the model in
    front of the *_aa arguments; the stages that only read the splat records have none."""
    xr = None if x is None else ctypes.byref(x)
    if cm is not None and cam is not None and not isinstance(cam, CamCmArgs):
        raise NotImplementedError("the camera gradients of include/gsr_cam.h have no camera_model form (include/gsr_cam_cm.h has)")
    if stage == "preprocess" and cm is not None:
        name = "gsr_forward_preprocess_leaf_cm" if leaf else "gsr_forward_preprocess_cm"
        lead = (ctypes.byref(cm), int(aa), xr)
    elif stage == "preprocess":
        name = "gsr_forward_preprocess_leaf" if leaf else "gsr_forward_preprocess"
        name, lead = (name + "_aa", (1, xr)) if aa else (name + "_aux", (xr,)) if x is not None else (name, ())
    elif stage == "gaussians" and cm is not None and cam is not None:
        name, lead = "gsr_backward_gaussians_cam_cm", (ctypes.byref(cm), int(aa), opacities if aa else None, xr, ctypes.byref(cam))
    elif stage == "gaussians" and cm is not None:
        name, lead = "gsr_backward_gaussians_cm", (ctypes.byref(cm), int(aa), opacities if aa else None, xr)
    elif stage == "gaussians" and cam is not None:
        name, lead = "gsr_backward_gaussians_cam", (int(aa), opacities if aa else None, xr, ctypes.byref(cam))
    elif stage == "gaussians":
        name, lead = ("gsr_backward_gaussians_aa", (1, opacities, xr)) if aa else \
            ("gsr_backward_gaussians_aux", (xr,)) if x is not None else ("gsr_backward_gaussians", ())
    elif stage == "blend" and absgrad:
        name, lead = "gsr_backward_blend_abs", (xr, 1)
    else:
        name = {"render": "gsr_forward_render", "blend": "gsr_backward_blend"}[stage]
        name, lead = (name + "_aux", (xr,)) if x is not None else (name, ())
    return getattr(L, name), lead


# ---- the forward of every variant ------------------------------------------------------------------------------------------------
def run_forward(leaf, mode, antialiasing, background, named, degree, M, W, H, scale_modifier, tan_fovx, tan_fovy, prefiltered, debug,
                camera_model=None):
    """Validate, allocate, preprocess, read the count back, allocate the binning state, render.
    named: the tensor arguments of the preprocess entry point in its order, as (tensor, name in error messages): the Gaussians first
    (five tensors, means3D leading, before scale_modifier; the rest after it), then viewmatrix, projmatrix, campos.
    mode: None, or aux_mode() of the depth and alpha maps to produce.
    camera_model: None, or a checked CameraModel (include/gsr_camera_model.h): projmatrix, tan_fovx and tan_fovy are then ignored.
    -> (num_rendered, out_color (3,H,W) f32, radii (P,) i32, geomBuffer, binningBuffer, imgBuffer, the contiguous tensors of `named`,
        () or (depth (1,H,W), alpha (1,H,W), auxBuffer))"""
    aa = aa_flag(antialiasing)
    means3D = named[0][0]
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")  # rasterize_points.cu:60-63
    if not means3D.is_cuda:
        raise RuntimeError("means3D must be a HIP (cuda) tensor; the HIP rasterizer has no CPU path")
    L = lib()
    dev = means3D.device
    P, H, W = int(means3D.size(0)), int(H), int(W)
    tensors = [_dev_f32(t, dev, n) for t, n in named]
    background = _dev_f32(background, dev, "bg")
    byte = dict(dtype=torch.uint8, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        alloc = torch.zeros if P == 0 else torch.empty   # the kernels write every element; nothing is launched for P == 0
        out_color = alloc((3, H, W), **f32)
        radii = torch.empty((P,), dtype=torch.int32, device=dev)
        maps = () if mode is None else (alloc((1, H, W), **f32), alloc((1, H, W), **f32))
        if P == 0:  # rasterize_points.cu:94
            e = torch.empty((0,), **byte)
            return 0, out_color, radii, e, e.clone(), e.clone(), tensors, maps and maps + (e.clone(),)
        geom = torch.empty((L.gsr_geometry_bytes(P),), **byte)
        img = torch.empty((L.gsr_image_bytes(W, H),), **byte)
        x = None
        if mode is not None:
            x = AuxArgs()
            x.mode = mode   # all that preprocess reads of it; the outputs are set once the count is known
        preprocess, pre_lead = _entry(L, "preprocess", leaf, x, aa, cm=camera_model_args(camera_model))
        render, ren_lead = _entry(L, "render", leaf, x)
        R = _i64(0)
        stream, dbg = _stream(dev), _dbg(debug)
        p = [_ptr(t) for t in tensors]
        _check(preprocess(*pre_lead, P, int(degree), int(M), W, H, *p[:5], float(scale_modifier), *p[5:], float(tan_fovx),
                          float(tan_fovy), int(bool(prefiltered)), _ptr(radii), _ptr(geom), ctypes.byref(R), stream, dbg))
        R = int(R.value)
        binning = torch.empty((L.gsr_binning_bytes(P, R, W, H),), **byte)
        if x is not None:
            maps += (torch.empty((L.gsr_aux_bytes(R, W, H),), **byte),)
            x.out_depth, x.out_alpha, x.scratch = (_ptr(t) for t in maps)
        _check(render(*ren_lead, P, R, W, H, _ptr(background), _ptr(radii), _ptr(geom), _ptr(binning), _ptr(img), _ptr(out_color),
                      stream, dbg))
    return R, out_color, radii, geom, binning, img, tensors, maps


def _forward_plain(mode, antialiasing, background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                   viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug,
                   cm=None):
    """The reference's argument list (rasterize_points.cu:38-59) -> run_forward()'s, in gsr_forward_preprocess's order."""
    r = run_forward(False, mode, antialiasing, background,
                    ((means3D, "means3D"), (sh, "shs"), (colors, "colors_precomp"), (opacity, "opacities"), (scales, "scales"),
                     (rotations, "rotations"), (cov3D_precomp, "cov3D_precomp"), (viewmatrix, "viewmatrix"),
                     (projmatrix, "projmatrix"), (campos, "campos")),
                    degree, int(sh.size(1)) if sh.numel() != 0 else 0, image_width, image_height, scale_modifier, tan_fovx,
                    tan_fovy, prefiltered, debug, camera_model(cm))
    return r[:6] + r[7]


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                        viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                        prefiltered, debug, *, antialiasing=False, camera_model=None):
    """-> (num_rendered, out_color (3,H,W) f32, radii (P,) i32, geomBuffer, binningBuffer, imgBuffer)
    antialiasing: the screen-space filter (include/gsr_aa.h): the splat records carry opacity * rho
    camera_model: a CameraModel (include/gsr_camera_model.h): projmatrix, tan_fovx and tan_fovy are then ignored"""
    return _forward_plain(None, antialiasing, background, means3D, colors, opacity, scales, rotations, scale_modifier,
                          cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                          prefiltered, debug, camera_model)


def rasterize_gaussians_depth_alpha(depth_alpha, background, means3D, colors, opacity, scales, rotations, scale_modifier,
                                    cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh,
                                    degree, campos, prefiltered, debug, *, antialiasing=False, camera_model=None):
    """rasterize_gaussians() with the depth and alpha maps of mode `depth_alpha` ("depth" / "invdepth") from the same blend pass
    -> (num_rendered, out_color, radii, geomBuffer, binningBuffer, imgBuffer, depth (1,H,W), alpha (1,H,W), auxBuffer).
    Colour, radii and the state buffers are bit-identical with rasterize_gaussians()'s (with the same `antialiasing`)."""
    return _forward_plain(aux_mode(depth_alpha), antialiasing, background, means3D, colors, opacity, scales, rotations,
                          scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh,
                          degree, campos, prefiltered, debug, camera_model)


# ---- the backward of every variant -----------------------------------------------------------------------------------------------
def backward_scratch(P, R, device):
    """The scratch of one backward (gsr_backward_args.scratch); hand it back with release_scratch() once the calls are enqueued."""
    return torch.empty((lib().gsr_backward_scratch_bytes(int(P), int(R)),), dtype=torch.uint8, device=device)


def release_scratch(scratch, device):
    scratch.record_stream(torch.cuda.current_stream(device))


def aux_backward_args(mode, scratch, dL_ddepth, dL_dalpha, device):
    """AuxArgs of a backward: dL_ddepth / dL_dalpha (1,H,W) or (H,W) or None (= zero).  The tensors must stay alive until the calls
    that use the struct have been enqueued; the contiguous copies are kept on the struct."""
    x = AuxArgs()
    x.mode = aux_mode(mode)
    keep = []
    for name, t in (("dL_ddepth", dL_ddepth), ("dL_dalpha", dL_dalpha)):
        if t is not None:
            t = _dev_f32(t, device, name)
            keep.append(t)
        setattr(x, name, _ptr(t))
    x.scratch = _ptr(scratch)
    x._keep = keep
    return x


def run_backward(a, scratch, device, x=None, opacities=None, parts=None, before_part=None, after_part=None, cam=None, absgrad=None,
                 features=None, distortion=None, median=None, camera_model=None):
    """The two-stage backward of a filled BackwardArgs `a` (inputs, outputs, stats; `scratch` is the tensor behind a.scratch): the
    blend pass, then the per-Gaussian pass for every (first, count) of `parts` (default: all Gaussians at once), writing rows from
    `first` on.  x: AuxArgs of a backward with map gradients, or None; opacities: the forward's opacity input (tensor or address; the
    logits in leaf mode) when the screen-space filter was on, else None; before_part(k) / after_part(k): called around part k's pass
    (view_parallel.py sets the part's output pointers and starts its collectives there).  cam: CamArgs (camera_target("cam", ...)) when
    the per-Gaussian pass shall also produce the camera gradients; it runs over all Gaussians at once, so not with `parts`.  With
    camera_model it is the CamCmArgs (camera_target("cm", ...)) of the camera gradients under that model.
    absgrad: AbsgradArgs (absgrad_tensors()) when the blend shall keep the per-pixel moduli of dL/dmean2D and a fold pass behind it
    shall overwrite abs_mean2D and add into abs_gradient_accum (include/gsr_absgrad.h); not with `parts` either.
    features: FeatureBackward (include/gsr_features.h) when a feature map took part in the loss: its pass runs between the blend (and
    the absgrad fold) and the per-Gaussian parts, adds the map's share of dL/dmean2D, dL/dconic and dL/dopacity into the slots and
    leaves dL/dfeatures in features.grad.  The slots are complete before the first part runs, so x, opacities, cam, absgrad and parts
    work unchanged.
    distortion: DistortionBackward (include/gsr_distortion.h) when the distortion map took part in the loss: its pass runs at the same
    place, behind the features', and adds into the slots' words 0..5 and 9 -- x (the AuxArgs) is then required, so that the aux
    kernels write and chain word 9.
    median: MedianBackward (include/gsr_median.h) when the median-depth map took part in the loss: its pass runs at the same place and
    adds into the slots' word 9 alone; x is required as for distortion.
    camera_model: the checked CameraModel of the forward (include/gsr_camera_model.h), or None."""
    if distortion is not None and x is None:
        raise RuntimeError("run_backward: the distortion map's backward needs the depth-and-alpha kernels (x is None)")
    if median is not None and x is None:
        raise RuntimeError("run_backward: the median-depth map's backward needs the depth-and-alpha kernels (x is None)")
    if cam is not None and parts is not None:
        raise NotImplementedError("camera gradients need the whole scene in one per-Gaussian pass: not with `parts`")
    if absgrad is not None and parts is not None:
        raise NotImplementedError("absolute gradients have no part-by-part form")
    L = lib()
    ra = ctypes.byref(a)
    blend, lead = _entry(L, "blend", x=x, absgrad=absgrad is not None)
    _check(blend(ra, *lead))
    if absgrad is not None:   # right behind the blend, while the slots are still in cache
        _check(L.gsr_absgrad_fold(ra, ctypes.byref(absgrad), 0, a.P))
    if features is not None:
        features.run(a, device, into_slots=True)
    if distortion is not None:
        distortion.run(a, device)
    if median is not None:
        median.run(a, device)
    aa = opacities is not None
    if aa and not isinstance(opacities, int):
        opacities = _ptr(_dev_f32(opacities, device, "opacities"))
    gaussians, lead = _entry(L, "gaussians", x=x, aa=aa, opacities=opacities, cam=cam, cm=camera_model_args(camera_model))
    for k, (first, count) in enumerate(((0, a.P),) if parts is None else parts):
        if before_part is not None:
            before_part(k)
        _check(gaussians(ra, *lead, int(first), int(count), int(first)))
        if after_part is not None:
            after_part(k)
    release_scratch(scratch, device)


def _backward_plain(who, aux, args, lean, skip_sh, debug_out, stats, antialiasing, opacities, camera_grads=False, absgrad=None,
                    features=None, distortion=None, median=None, cm=None, camera_model_grads=False):
    """rasterize_gaussians_backward() / rasterize_gaussians_backward_depth_alpha(): args are the reference's 21 (rasterize_points.cu:
    132-153), aux is None or (depth_alpha, auxBuffer, dL_ddepth, dL_dalpha)."""
    (background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
     dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug) = args
    aa = aa_flag(antialiasing)
    if aa and opacities is None:
        raise RuntimeError(f"{who}: antialiasing=True needs the forward's opacities")
    cm = camera_model(cm)
    camera_model_excludes(cm, camera_flag(camera_grads))
    if not isinstance(camera_model_grads, bool):
        raise TypeError(f"{who}: camera_model_grads must be True or False here, got {camera_model_grads!r}")
    kind = "cam" if camera_grads else "cm" if camera_model_grads_arg(camera_model_grads, cm) else None
    cam, cam_grads = None, ()
    L = lib()
    dev = means3D.device
    P = int(means3D.size(0))
    H, W = int(dL_dout_color.size(1)), int(dL_dout_color.size(2))
    M = int(sh.size(1)) if sh.numel() != 0 else 0
    f32 = dict(dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        # every element is written by the kernels (no zero-fill pass, unlike rasterize_points.cu:168-178)
        alloc = torch.zeros if P == 0 else torch.empty
        dL_dmeans3D = alloc((P, 3), **f32)
        dL_dmeans2D = alloc((P, 3), **f32)
        skip_sh = bool(skip_sh) and M > 0
        lean = bool(lean) and debug_out is None
        none = torch.empty((0,), **f32)
        dL_dcolors = alloc((P, 3), **f32) if (not lean or colors.numel() != 0 or skip_sh) else none
        dL_dconic = alloc((P, 2, 2), **f32) if not lean else none
        dL_dopacity = alloc((P, 1), **f32)
        dL_dcov3D = alloc((P, 6), **f32) if (not lean or cov3D_precomp.numel() != 0) else none
        dL_dsh = None if skip_sh else alloc((P, M, 3), **f32)
        dL_dscales = alloc((P, 3), **f32)
        dL_drotations = alloc((P, 4), **f32)
        if P != 0:
            background, means3D, colors, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, dL_dout_color, sh, campos = (
                _dev_f32(t, dev, n) for t, n in (
                    (background, "bg"), (means3D, "means3D"), (colors, "colors_precomp"), (scales, "scales"), (rotations, "rotations"),
                    (cov3D_precomp, "cov3D_precomp"), (viewmatrix, "viewmatrix"), (projmatrix, "projmatrix"),
                    (dL_dout_color, "dL_dout_color"), (sh, "shs"), (campos, "campos")))
            scratch = backward_scratch(P, R, dev)
            if kind is not None:
                cam, cam_grads = camera_target(kind, P, dev)
            ab = None if absgrad is None else absgrad_tensors(absgrad, P, dev)
            if stats is None and not aa and aux is None and cam is None and ab is None and features is None and cm is None:   # nothing but the reference's backward: one call for both stages
                _check(L.gsr_backward(P, int(degree), M, int(R), W, H, _ptr(background), _ptr(means3D), _ptr(sh), _ptr(colors),
                                      _ptr(scales), float(scale_modifier), _ptr(rotations), _ptr(cov3D_precomp),
                                      _ptr(viewmatrix), _ptr(projmatrix), _ptr(campos), float(tan_fovx), float(tan_fovy),
                                      _ptr(radii), _ptr(geomBuffer), _ptr(binningBuffer), _ptr(imageBuffer), _ptr(scratch),
                                      _ptr(dL_dout_color), _ptr(dL_dmeans2D), _ptr(dL_dconic), _ptr(dL_dopacity),
                                      _ptr(dL_dcolors), _ptr(dL_dmeans3D), _ptr(dL_dcov3D), _ptr(dL_dsh), _ptr(dL_dscales),
                                      _ptr(dL_drotations), _stream(dev), _dbg(debug)))
                release_scratch(scratch, dev)
            else:
                a = backward_args(P=P, D=int(degree), M=M, R=int(R), W=W, H=H, leaf=0, background=background, means3D=means3D,
                                  shs=sh, colors_precomp=colors, scales=scales, scale_modifier=scale_modifier,
                                  rotations=rotations, cov3D_precomp=cov3D_precomp, viewmatrix=viewmatrix,
                                  projmatrix=projmatrix, cam_pos=campos, tan_fovx=tan_fovx, tan_fovy=tan_fovy, radii=radii,
                                  geometry=geomBuffer, binning=binningBuffer, image=imageBuffer, scratch=scratch,
                                  dL_dpix=dL_dout_color, debug=debug, device=dev)
                set_backward_outputs(a, dL_dmean2D=dL_dmeans2D, dL_dconic=dL_dconic, dL_dopacity=dL_dopacity,
                                     dL_dcolor=dL_dcolors, dL_dmean3D=dL_dmeans3D, dL_dcov3D=dL_dcov3D, dL_dsh=dL_dsh,
                                     dL_dscale=dL_dscales, dL_drot=dL_drotations)
                set_backward_stats(a, stats, P, dev)
                run_backward(a, scratch, dev, None if aux is None else aux_backward_args(*aux, dev), opacities if aa else None, cam=cam,
                             absgrad=ab, features=features, distortion=distortion, median=median, camera_model=cm)
        elif kind is not None:   # no Gaussian: nothing is launched
            cam, cam_grads = camera_target(kind, 0, dev)
    if debug_out is not None:
        debug_out["dL_dconic"] = dL_dconic
    return (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations) + tuple(cam_grads)


def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree,
                                 campos, geomBuffer, R, binningBuffer, imageBuffer, debug, *, lean=False, skip_sh=False,
                                 debug_out=None, stats=None, antialiasing=False, opacities=None, camera_grads=False, absgrad=None,
                                 features=None, camera_model=None, camera_model_grads=False):
    """-> (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)

    The 21 positional arguments and the tuple are the reference extension's.  Keyword-only extras (all per call,
    nothing is kept between calls):
      lean      outputs that autograd would drop anyway (dL_dcolors when the colours came from SH, dL_dcov3D when the
                covariances came from scales/rotations, the internal dL_dconic) are not computed: empty tensors
      skip_sh   view-parallel mode: dL_dsh is not produced (None) and dL_dcolors carries the clamp-masked dL/dRGB
                of the view, the input of sh_grad_from_views()
      debug_out dict that receives the internal "dL_dconic" tensor (tests)
      stats     (xyz_gradient_accum, denom, max_radii2D) float32 [P] tensors updated in place for the Gaussians
                visible in this view (train.py:157-159, gaussian_model.py:599-602); any of them may be None
      antialiasing  the backward of an antialiasing=True forward; `opacities` is then its opacity input (include/gsr_aa.h)
      camera_grads  True: three more results behind the eight, dL_dviewmatrix (4,4), dL_dprojmatrix (4,4) and dL_dcampos (3,) of the
                    camera tensors as the kernels read them (include/gsr_cam.h)
      absgrad   (abs_mean2D [P, 2], abs_gradient_accum [P]) float32 tensors, either None: the first is overwritten with the sums over
                the pixels of |dL_p/dmean2D| per component, the second gets their norm added for the visible Gaussians
                (include/gsr_absgrad.h)
      features  FeatureBackward(features, dL_dfeature_map): the feature map of features_forward() took part in the loss; its share
                of the geometry gradients is in the eight results, dL/dfeatures is left in features.grad (include/gsr_features.h)
      camera_model  the CameraModel of the forward (include/gsr_camera_model.h); not with camera_grads (camera_model_grads below)
      camera_model_grads  True (with camera_model): three more results behind the eight, dL_dviewmatrix (4,4), dL_dintrinsics (4,)
                    = dL/d(fx, fy, cx, cy) and dL_dcampos (3,) (include/gsr_cam_cm.h)"""
    return _backward_plain("rasterize_gaussians_backward", None,
                           (background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                            projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer,
                            imageBuffer, debug), lean, skip_sh, debug_out, stats, antialiasing, opacities, camera_grads, absgrad,
                           features, cm=camera_model, camera_model_grads=camera_model_grads)


def rasterize_gaussians_backward_depth_alpha(depth_alpha, background, means3D, radii, colors, scales, rotations, scale_modifier,
                                             cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh,
                                             degree, campos, geomBuffer, R, binningBuffer, imageBuffer, auxBuffer, dL_ddepth,
                                             dL_dalpha, debug, *, stats=None, antialiasing=False, opacities=None,
                                             camera_grads=False, absgrad=None, features=None, distortion=None, median=None,
                                             camera_model=None, camera_model_grads=False):
    """rasterize_gaussians_backward() of a rasterize_gaussians_depth_alpha() forward, with dL/dD and dL/dA (1,H,W) or None on
    top of dL/dpix -> the same eight gradients (the lean set: dL_dcolors only for precomputed colours, dL_dcov3D only for
    precomputed covariances, as rasterize_gaussians_backward(lean=True)).  antialiasing / opacities / camera_grads / absgrad /
    features: as there.  distortion: DistortionBackward(state, dL_ddistortion) when the map of distortion_forward() took part in
    the loss; its share is in the eight results, dL/dv chained to dL_dmeans3D (include/gsr_distortion.h).  median:
    MedianBackward(state, dL_dmedian_depth) when the median-depth map of median_forward() did; its dL/dv is chained the same way
    (include/gsr_median.h).  camera_model, camera_model_grads: as there."""
    return _backward_plain("rasterize_gaussians_backward_depth_alpha", (depth_alpha, auxBuffer, dL_ddepth, dL_dalpha),
                           (background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                            projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer,
                            imageBuffer, debug), True, False, None, stats, antialiasing, opacities, camera_grads, absgrad, features,
                           distortion, median, camera_model, camera_model_grads)


# ---- blend-weight statistics of a forward's state (include/gsr_contrib.h) -----------------------------------------------------------
def contrib_stat_tensors(stats, P):
    """Checks stats = (weight_sum f32, weight_max f32, pixel_count i32), [P] each, any of them None -> their device.  No kernel and no
    library is touched: CPU tensors, wrong dtypes and wrong shapes are refused first."""
    if not isinstance(stats, (tuple, list)) or len(stats) != 3 or all(t is None for t in stats):
        raise RuntimeError("contrib_stats must be (weight_sum, weight_max, pixel_count) with at least one tensor")
    dev = None
    for name, t, dt in zip(("weight_sum", "weight_max", "pixel_count"), stats, (torch.float32, torch.float32, torch.int32)):
        if t is None:
            continue
        tn = str(dt).replace("torch.", "")
        if t.dtype != dt:
            raise RuntimeError(f"{name} must be {tn} (got {t.dtype})")
        if tuple(t.shape) != (P,) or not t.is_contiguous():
            raise RuntimeError(f"{name} must be a contiguous {tn} tensor with P = {P} elements (got shape {tuple(t.shape)})")
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a HIP (cuda) tensor (got {t.device}); the HIP rasterizer has no CPU path")
        dev = t.device if dev is None else dev
        if t.device != dev:
            raise RuntimeError(f"{name} must be on {dev} (got {t.device})")
    return dev


def contrib_pixel_weight(pixel_weight, W, H, device):
    """The per-pixel weight map m of the weight sums: (H, W) or (1, H, W) float32 on `device`, or None (= 1) -> contiguous or None."""
    if pixel_weight is None:
        return None
    if tuple(pixel_weight.shape) not in ((H, W), (1, H, W)):
        raise RuntimeError(f"pixel_weight must have shape ({H}, {W}) or (1, {H}, {W}), got {tuple(pixel_weight.shape)}")
    if pixel_weight.dtype != torch.float32:
        raise RuntimeError(f"pixel_weight must be float32 (got {pixel_weight.dtype})")
    return _dev_f32(pixel_weight, device, "pixel_weight")


def gaussian_contributions(geomBuffer, binningBuffer, imgBuffer, num_rendered, P, W, H, stats, pixel_weight=None, debug=0):
    """Per-Gaussian blend-weight statistics of the view whose forward left the three state buffers (of any variant), updated in place:
    weight_sum += sum_p m(p) w(p), weight_max = max(itself, max_p w(p)), pixel_count += pixels blended into, with w = alpha * T of the
    forward and m = pixel_weight ((H, W) or (1, H, W); None = 1).  Gaussians that blended nowhere keep their values.  No gradients, no
    atomics; nothing of the state is written, so the backward of the same forward may still follow."""
    P, R, W, H = int(P), int(num_rendered), int(W), int(H)
    dev = contrib_stat_tensors(stats, P)
    m = contrib_pixel_weight(pixel_weight, W, H, dev)
    for name, t in (("geomBuffer", geomBuffer), ("binningBuffer", binningBuffer), ("imgBuffer", imgBuffer)):
        if t.numel() != 0 and t.device != dev:
            raise RuntimeError(f"{name} must be on {dev} (got {t.device}); the HIP rasterizer has no CPU path")
    L = lib()
    with torch.cuda.device(dev):
        scratch = None
        if P > 0 and R > 0:
            scratch = torch.empty((L.gsr_contrib_scratch_bytes(P, R),), dtype=torch.uint8, device=dev)
        _check(L.gsr_contributions(P, R, W, H, _ptr(geomBuffer), _ptr(binningBuffer), _ptr(imgBuffer), _ptr(m), *(_ptr(t) for t in stats),
                                   _ptr(scratch), _stream(dev), _dbg(debug)))


# ---- K blended feature channels (include/gsr_features.h) ---------------------------------------------------------------------------
def feature_tensor(features, P, device=None):
    """Checks the `features` keyword: a float32 (P, K) HIP tensor, K >= 1 -> K.  No kernel and no library is touched: anything but a
    tensor raises TypeError; a CPU tensor, a wrong dtype, a wrong shape or a wrong device RuntimeError; a (P, M, K) tensor of SH
    coefficients NotImplementedError (view-dependent features are evaluated by the caller)."""
    if not isinstance(features, torch.Tensor):
        raise TypeError(f"features must be a float32 (P, K) tensor or None, got {type(features).__name__}")
    if features.dim() == 3:
        raise NotImplementedError("SH-evaluated features are not supported: evaluate them per view and pass the (P, K) result")
    if features.dtype != torch.float32:
        raise RuntimeError(f"features must be float32 (got {features.dtype})")
    if features.dim() != 2 or int(features.size(0)) != int(P) or int(features.size(1)) < 1:
        raise RuntimeError(f"features must have shape (P, K) with P = {int(P)} and K >= 1 (got {tuple(features.shape)})")
    if not features.is_cuda:
        raise RuntimeError(f"features must be a HIP (cuda) tensor (got {features.device}); the HIP rasterizer has no CPU path")
    if device is not None and features.device != device:
        raise RuntimeError(f"features must be on {device} (got {features.device})")
    return int(features.size(1))


def features_forward(geomBuffer, binningBuffer, imgBuffer, num_rendered, P, W, H, features, debug=0):
    """feature_map (K, H, W) = sum_i features[i] alpha_i T_i of the view whose forward (of any variant) left the three state buffers:
    the colour pass's own weights bit for bit, no background term, zeros where nothing blends.  Nothing of the state is written."""
    P, R, W, H = int(P), int(num_rendered), int(W), int(H)
    K = feature_tensor(features, P)
    dev = features.device
    features = features.contiguous()
    with torch.cuda.device(dev):
        out = (torch.zeros if P == 0 else torch.empty)((K, H, W), dtype=torch.float32, device=dev)
        if P > 0:
            _check(lib().gsr_features_forward(P, R, W, H, K, _ptr(geomBuffer), _ptr(binningBuffer), _ptr(imgBuffer), _ptr(features),
                                              _ptr(out), _stream(dev), _dbg(debug)))
    return out


class FeatureBackward:
    """The feature map's part of one backward: features (P, K) and dL_dfeature_map (K, H, W).  run() leaves dL/dfeatures (P, K) in
    .grad -- every element written, zeros for Gaussians without a hit."""

    def __init__(self, features, dL_dmap):
        self.K = feature_tensor(features, features.size(0))
        dev = features.device
        self.features = features.contiguous()
        self.dL_dmap = _dev_f32(dL_dmap, dev, "dL_dfeature_map")
        if self.dL_dmap.dim() != 3 or int(self.dL_dmap.size(0)) != self.K:
            raise RuntimeError(f"dL_dfeature_map must have shape ({self.K}, H, W), got {tuple(self.dL_dmap.shape)}")
        self.grad = None

    def run(self, a, device, into_slots):
        """a: the BackwardArgs of the colour backward (into_slots: its blend has run, its per-Gaussian pass has not), or one that
        holds the sizes, the three state buffers, stream and debug alone (not into_slots: a.scratch is not touched)."""
        L = lib()
        P, R = int(a.P), int(a.num_rendered)
        if tuple(self.dL_dmap.shape[1:]) != (int(a.height), int(a.width)):
            raise RuntimeError(f"dL_dfeature_map must have shape ({self.K}, {a.height}, {a.width}), got {tuple(self.dL_dmap.shape)}")
        self.grad = (torch.zeros if P == 0 else torch.empty)((P, self.K), dtype=torch.float32, device=device)
        if P == 0:
            return self.grad
        scratch = None
        if R > 0:
            scratch = torch.empty((L.gsr_features_scratch_bytes(P, R, self.K),), dtype=torch.uint8, device=device)
        _check(L.gsr_features_backward(ctypes.byref(a), self.K, _ptr(self.features), _ptr(self.dL_dmap), _ptr(self.grad), _ptr(scratch),
                                       1 if into_slots else 0))
        if scratch is not None:
            release_scratch(scratch, device)
        return self.grad


def features_backward_only(geomBuffer, binningBuffer, imgBuffer, num_rendered, P, W, H, features, dL_dmap, debug=0):
    """dL/dfeatures (P, K) alone, for features on a frozen scene: no colour backward, no gradient slots, no geometry gradient."""
    fb = FeatureBackward(features, dL_dmap)
    dev = features.device
    a = BackwardArgs()
    a.P, a.num_rendered, a.width, a.height = int(P), int(num_rendered), int(W), int(H)
    a.geometry, a.binning, a.image = _ptr(geomBuffer), _ptr(binningBuffer), _ptr(imgBuffer)
    a.debug = _dbg(debug)
    with torch.cuda.device(dev):
        a.stream = _stream(dev)
        return fb.run(a, dev, into_slots=False)


# ---- the depth-distortion map (include/gsr_distortion.h) ---------------------------------------------------------------------------
def distortion_flag(distortion, depth_alpha=None):
    """Checks the `distortion` keyword: a bool (anything else raises TypeError), and True only together with a depth_alpha mode
    (ValueError: the depth value v_i lives only in the records of a depth-and-alpha forward) -> the bool.  No library is touched."""
    if not isinstance(distortion, bool):
        raise TypeError(f"distortion must be a bool, got {type(distortion).__name__}")
    if distortion and depth_alpha is None:
        raise ValueError('distortion=True needs depth_alpha="depth" or "invdepth": the depth values v_i of the map live only in the '
                         "records of a depth-and-alpha forward")
    return distortion


def distortion_forward(geomBuffer, binningBuffer, imgBuffer, num_rendered, P, W, H, debug=0):
    """-> (distortion (1, H, W), state (3, H, W)): Dist = sum_{j<i} w_i w_j (v_i - v_j)^2 of the view whose depth-and-alpha forward
    left the three state buffers, with the colour pass's own weights and the records' depth values, accumulated centred; state = the
    per-pixel (A, mu, S) that DistortionBackward reads.  Zeros where fewer than two Gaussians blend.  Nothing of the state buffers is
    written."""
    P, R, W, H = int(P), int(num_rendered), int(W), int(H)
    dev = imgBuffer.device
    if not imgBuffer.is_cuda:
        raise RuntimeError(f"imgBuffer must be a HIP (cuda) tensor (got {dev}); the HIP rasterizer has no CPU path")
    with torch.cuda.device(dev):
        alloc = torch.zeros if P == 0 else torch.empty
        out = alloc((1, H, W), dtype=torch.float32, device=dev)
        state = alloc((3, H, W), dtype=torch.float32, device=dev)
        if P > 0:
            _check(lib().gsr_distortion_forward(P, R, W, H, _ptr(geomBuffer), _ptr(binningBuffer), _ptr(imgBuffer), _ptr(out), _ptr(state),
                                                _stream(dev), _dbg(debug)))
    return out, state


class DistortionBackward:
    """The distortion map's part of one backward: the state distortion_forward() returned and dL_ddistortion (1, H, W) or (H, W).
    run() adds its share into the gradient slots between the aux blend and the per-Gaussian pass."""

    def __init__(self, state, dL_ddist):
        self.state = state
        self.dL_ddist = _dev_f32(dL_ddist, state.device, "dL_ddistortion")
        if tuple(self.dL_ddist.shape[-2:]) != tuple(state.shape[-2:]) or self.dL_ddist.numel() != state.numel() // 3:
            raise RuntimeError(f"dL_ddistortion must have shape (1, {state.size(1)}, {state.size(2)}), got {tuple(self.dL_ddist.shape)}")

    def run(self, a, device):
        if (int(a.height), int(a.width)) != tuple(self.state.shape[-2:]):
            raise RuntimeError(f"the distortion state is of a {tuple(self.state.shape[-2:])} image, the backward of {(a.height, a.width)}")
        if int(a.P) == 0:
            return
        _check(lib().gsr_distortion_backward(ctypes.byref(a), _ptr(self.state), _ptr(self.dL_ddist)))


# ---- the median-depth map and the per-pixel index maps (include/gsr_median.h) -------------------------------------------------------
def median_flag(median_depth, depth_alpha=None):
    """Checks the `median_depth` keyword: a bool (anything else raises TypeError), and True only together with a depth_alpha mode
    (ValueError: the depth value v_i lives only in the records of a depth-and-alpha forward) -> the bool.  No library is touched."""
    if not isinstance(median_depth, bool):
        raise TypeError(f"median_depth must be a bool, got {type(median_depth).__name__}")
    if median_depth and depth_alpha is None:
        raise ValueError('median_depth=True needs depth_alpha="depth" or "invdepth": the depth values v_i of the map live only in the '
                         "records of a depth-and-alpha forward")
    return median_depth


def index_map_tensors(index_maps, W, H, device=None):
    """Checks the `index_maps` keyword: None, or a 3-tuple (median_index int32, dominant_index int32, dominant_weight float32) of
    contiguous (H, W) or (1, H, W) HIP tensors on one device (`device` when given), any of them None but not all -> their device, or
    None for index_maps=None.  Anything but None or a 3-tuple raises TypeError, wrong tensors ValueError.  No kernel and no library is
    touched."""
    if index_maps is None:
        return None
    if not isinstance(index_maps, (tuple, list)) or len(index_maps) != 3:
        raise TypeError("index_maps must be a 3-tuple (median_index, dominant_index, dominant_weight), "
                        f"got {type(index_maps).__name__}" + (f" of {len(index_maps)}" if isinstance(index_maps, (tuple, list)) else ""))
    if all(t is None for t in index_maps):
        raise ValueError("index_maps needs at least one tensor")
    W, H = int(W), int(H)
    for name, t, dt in zip(("median_index", "dominant_index", "dominant_weight"), index_maps, (torch.int32, torch.int32, torch.float32)):
        if t is None:
            continue
        tn = str(dt).replace("torch.", "")
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a {tn} tensor or None, got {type(t).__name__}")
        if t.dtype != dt:
            raise ValueError(f"{name} must be {tn} (got {t.dtype})")
        if tuple(t.shape) not in ((H, W), (1, H, W)) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {tn} tensor of shape ({H}, {W}) or (1, {H}, {W}) (got shape {tuple(t.shape)})")
        if not t.is_cuda:
            raise ValueError(f"{name} must be a HIP (cuda) tensor (got {t.device}); the HIP rasterizer has no CPU path")
        device = t.device if device is None else device
        if t.device != device:
            raise ValueError(f"{name} must be on {device} (got {t.device})")
    return device


def median_forward(geomBuffer, binningBuffer, imgBuffer, num_rendered, P, W, H, index_maps=None, depth=True, debug=0):
    """-> (median_depth (1, H, W), state (H, W) int32), or (None, None) with depth=False: the median-depth map of the view whose
    forward left the three state buffers -- v of the last blended Gaussian in front of which the transmittance is above 0.5, the
    record's bits (all zeros after a forward without a depth_alpha mode) -- and the median's position in its tile's list per pixel
    (-1: nothing blended), which MedianBackward reads.  index_maps: None, or (median_index, dominant_index, dominant_weight) as
    index_map_tensors() checks them, overwritten in place by the same launch: the Gaussian id of the median, the id of the blended
    Gaussian with the largest weight alpha T (the first on a tie), -1 where nothing blends, and that weight.  debug:
    DEBUG_MEDIAN_FULL_WALK switches the early exit off.  Nothing of the state buffers is written."""
    P, R, W, H = int(P), int(num_rendered), int(W), int(H)
    dev = imgBuffer.device
    if not imgBuffer.is_cuda:
        raise RuntimeError(f"imgBuffer must be a HIP (cuda) tensor (got {dev}); the HIP rasterizer has no CPU path")
    index_map_tensors(index_maps, W, H, dev)
    maps = (None, None, None) if index_maps is None else tuple(index_maps)
    if not depth and index_maps is None:
        raise ValueError("median_forward: nothing is asked for (depth=False and index_maps=None)")
    with torch.cuda.device(dev):
        out = torch.empty((1, H, W), dtype=torch.float32, device=dev) if depth else None
        state = torch.empty((H, W), dtype=torch.int32, device=dev) if depth else None
        if P > 0:
            _check(lib().gsr_median_forward(P, R, W, H, _ptr(geomBuffer), _ptr(binningBuffer), _ptr(imgBuffer), _ptr(out), _ptr(maps[0]),
                                            _ptr(maps[1]), _ptr(maps[2]), _ptr(state), _stream(dev), _dbg(debug)))
        else:   # no Gaussian: nothing is launched
            for t, fill in ((out, 0), (state, -1), (maps[0], -1), (maps[1], -1), (maps[2], 0)):
                if t is not None:
                    t.fill_(fill)
    return out, state


class MedianBackward:
    """The median-depth map's part of one backward: the state median_forward() returned and dL_dmedian_depth (1, H, W) or (H, W).
    run() adds dL/dv into word 9 of the gradient slots between the aux blend and the per-Gaussian pass."""

    def __init__(self, state, dL_dmedian):
        self.state = state
        self.dL_dmedian = _dev_f32(dL_dmedian, state.device, "dL_dmedian_depth")
        if tuple(self.dL_dmedian.shape[-2:]) != tuple(state.shape[-2:]) or self.dL_dmedian.numel() != state.numel():
            raise RuntimeError(f"dL_dmedian_depth must have shape (1, {state.size(-2)}, {state.size(-1)}), got {tuple(self.dL_dmedian.shape)}")

    def run(self, a, device):
        if (int(a.height), int(a.width)) != tuple(self.state.shape[-2:]):
            raise RuntimeError(f"the median state is of a {tuple(self.state.shape[-2:])} image, the backward of {(a.height, a.width)}")
        if int(a.P) == 0:
            return
        _check(lib().gsr_median_backward(ctypes.byref(a), _ptr(self.state), _ptr(self.dL_dmedian)))


# ---- the normal map of render(normals=True) (include/gsr_normals.h, fused_geometry.py) ----------------------------------------------
NORMAL_SPACES = {"view": 0, "world": 1}   # GSR_NORMALS_VIEW / GSR_NORMALS_WORLD


def normals_flag(normals):
    """The `normals` keyword -> bool; anything but a bool raises TypeError, like `distortion`.  No library is touched."""
    if not isinstance(normals, bool):
        raise TypeError(f"normals must be a bool, got {type(normals).__name__}")
    return normals


# ---- the backward in two stages (include/gsr.h gsr_backward_blend / gsr_backward_gaussians) ------------------
def backward_args(*, P, D, M, R, W, H, leaf, background, means3D, shs, scales, scale_modifier, rotations, viewmatrix,
                  projmatrix, cam_pos, tan_fovx, tan_fovy, radii, geometry, binning, image, scratch, dL_dpix, debug, device,
                  shs_rest=None, colors_precomp=None, cov3D_precomp=None):
    """Input side of a gsr_backward_args; the gradient pointers are set with set_backward_outputs().  The tensors must
    stay alive (and contiguous float32 on `device`) until the calls that use the struct have been enqueued."""
    a = BackwardArgs()
    a.P, a.D, a.M, a.num_rendered, a.width, a.height, a.leaf = int(P), int(D), int(M), int(R), int(W), int(H), int(leaf)
    for name, t in (("background", background), ("means3D", means3D), ("shs", shs), ("shs_rest", shs_rest),
                    ("colors_precomp", colors_precomp), ("scales", scales), ("rotations", rotations),
                    ("cov3D_precomp", cov3D_precomp), ("viewmatrix", viewmatrix), ("projmatrix", projmatrix),
                    ("cam_pos", cam_pos), ("radii", radii), ("geometry", geometry), ("binning", binning), ("image", image),
                    ("scratch", scratch), ("dL_dpix", dL_dpix)):
        setattr(a, name, _ptr(t))
    a.scale_modifier, a.tan_fovx, a.tan_fovy = float(scale_modifier), float(tan_fovx), float(tan_fovy)
    a.stream = _stream(device)
    a.debug = _dbg(debug)
    return a


def set_backward_outputs(a, **ptrs):
    """ptrs: field name -> tensor (its data_ptr), int address, or None.  With out_row0 = first, an address is where
    the row of Gaussian `first` goes."""
    for name, t in ptrs.items():
        setattr(a, name, t if (t is None or isinstance(t, int)) else _ptr(t))


def set_backward_stats(a, stats, P, device):
    if stats is None:
        return
    for name, t in zip(("stat_xyz_gradient_accum", "stat_denom", "stat_max_radii2D"), stats):
        if t is None:
            continue
        if t.device != device or t.dtype != torch.float32 or t.numel() != P or not t.is_contiguous():
            raise RuntimeError(f"{name} must be a contiguous float32 tensor with P = {P} elements on {device}")
        setattr(a, name, t.data_ptr())


def backward_blend(a):
    _check(lib().gsr_backward_blend(ctypes.byref(a)))


def backward_gaussians(a, first, count, out_row0=0):
    _check(lib().gsr_backward_gaussians(ctypes.byref(a), int(first), int(count), int(out_row0)))


def sh_grad_from_views(means3D, cam_pos, dL_dRGB, degree, M, out=None):
    """dL_dsh (P,M,3) summed over V views from their clamp-masked dL/dRGB (V,P,3) and camera
    positions (V,3): include/gsr.h gsr_sh_grad_from_views.  out: optional contiguous (P,M,3) destination (a row
    range of a larger tensor when the caller works part by part)."""
    if not means3D.is_cuda:
        raise RuntimeError("means3D must be a HIP (cuda) tensor; the HIP rasterizer has no CPU path")
    L = lib()
    dev = means3D.device
    P, V = int(means3D.size(0)), int(dL_dRGB.size(0))
    assert dL_dRGB.shape == (V, P, 3) and cam_pos.shape == (V, 3)
    # views may be strided along dim 0 (blocks of an all-gather with a trailer row): consumed in place
    if P and not (dL_dRGB.stride(2) == 1 and dL_dRGB.stride(1) == 3 and (V <= 1 or dL_dRGB.stride(0) >= 3 * P)):
        dL_dRGB = dL_dRGB.contiguous()
    view_stride = int(dL_dRGB.stride(0)) if (P and V > 1) else 0
    if dL_dRGB.device != dev or dL_dRGB.dtype != torch.float32:
        raise RuntimeError("dL_dRGB must be a float32 tensor on the device of means3D")
    means3D, cam_pos = (_dev_f32(t, dev, n) for t, n in ((means3D, "means3D"), (cam_pos, "cam_pos")))
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((P, M, 3), dtype=torch.float32, device=dev)
        elif out.shape != (P, M, 3) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
            raise RuntimeError("sh_grad_from_views: out must be a contiguous float32 (P,M,3) tensor on the device of means3D")
        _check(L.gsr_sh_grad_from_views(P, int(degree), int(M), V, _ptr(means3D), _ptr(cam_pos), _ptr(dL_dRGB), view_stride,
                                        _ptr(out), _stream(dev)))
    return out


def mark_visible(means3D, viewmatrix, projmatrix):
    """-> bool (P,)"""
    if not means3D.is_cuda:
        raise RuntimeError("means3D must be a HIP (cuda) tensor; the HIP rasterizer has no CPU path")
    L = lib()
    dev = means3D.device
    P = int(means3D.size(0))
    present = torch.zeros((P,), dtype=torch.bool, device=dev)
    if P != 0:
        means3D = _dev_f32(means3D, dev, "means3D")
        viewmatrix = _dev_f32(viewmatrix, dev, "viewmatrix")
        projmatrix = _dev_f32(projmatrix, dev, "projmatrix")
        with torch.cuda.device(dev):
            _check(L.gsr_mark_visible(P, _ptr(means3D), _ptr(viewmatrix), _ptr(projmatrix), _ptr(present), _stream(dev)))
    return present


def thread_release():
    """include/gsr.h gsr_thread_release: frees the calling thread's helper stream, events and pinned buffer."""
    _check(lib().gsr_thread_release())


# ---- introspection helpers (tests / bench; not part of the reference surface) ----------------------
def geometry_layout(P):
    o = GeometryLayout()
    _check(lib().gsr_geometry_layout_of(P, ctypes.byref(o)))
    return o


def image_layout(W, H):
    o = ImageLayout()
    _check(lib().gsr_image_layout_of(W, H, ctypes.byref(o)))
    return o


def binning_layout(P, R, W, H):
    o = BinningLayout()
    _check(lib().gsr_binning_layout_of(P, R, W, H, ctypes.byref(o)))
    return o


def profile_begin(only=None, device=None):
    """Start recording per-stage HIP events for calls made on `device`'s current stream; `only` = name of the
    single stage to record."""
    stream = _stream(torch.device("cuda", torch.cuda.current_device()) if device is None else device)
    _check(lib().gsr_profile_begin_only(stream, None if only is None else only.encode()))


def profile_end(capacity=256, device=None):
    stream = _stream(torch.device("cuda", torch.cuda.current_device()) if device is None else device)
    arr = (KernelTime * capacity)()
    n = lib().gsr_profile_end(stream, arr, capacity)
    return [(arr[k].name.decode(), float(arr[k].ms)) for k in range(n)]


def aux_layout(R, W, H):
    lay = AuxLayout()
    _check(lib().gsr_aux_layout_of(int(R), int(W), int(H), ctypes.byref(lay)))
    return {n: getattr(lay, n) for n, _ in AuxLayout._fields_}
