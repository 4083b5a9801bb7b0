"""The 3D smoothing filter of Mip-Splatting ("Mip-Splatting: Alias-free 3D Gaussian Splatting") as fused HIP kernels
(include/gsr_filter3d.h), on the optimiser's leaves as fused_params lays them out -- the half of the method that `antialiasing=True`
(the screen-space filter) leaves out:

    compute_filter_3d(xyz, cameras, per_camera=False)    GaussianModel.compute_3D_filter: the per-Gaussian low-pass radius (P,1) from
                                                         the closest training camera that sees the Gaussian; three launches for any
                                                         number of cameras
    filtered_activations(opacity, scaling, filter_3d)    get_opacity_with_3D_filter / get_scaling_with_3D_filter, differentiable
                                                         w.r.t. the two leaves: one launch forward, one backward
    reset_opacity(optimizer, filter_3d, max_opacity)     the opacity reset under the filter, in place, moments zeroed: one launch
    baked_leaves(opacity, scaling, filter_3d)            save_fused_ply: the leaves for a viewer that does not know the filter

    filter_3d = compute_filter_3d(pc._xyz, train_cameras)        # after every densification, and every 100 iterations after it ends
    out = render(camera, pc, pipe, bg, filter_3d=filter_3d)      # gaussian_renderer.render applies filtered_activations

When the filter is recomputed stays with the training loop.  No floating-point atomics and no read-back: every result is bitwise
reproducible, the sweep under any permutation of the cameras.  HIP tensors only (no CPU fallback).
"""
import ctypes
import functools
import math

import torch

from diff_gaussian_rasterization import _C, _binding
from diff_gaussian_rasterization._binding import ptr

THREADS = 256            # include/gsr_filter3d.h GSR_FILTER3D_THREADS
CAMERA_FLOATS = 20       # GSR_FILTER3D_CAMERA_FLOATS
UNSEEN = 100000.0        # GSR_FILTER3D_UNSEEN: the filter of every row where no row is valid in any camera


class FilterCamera(ctypes.Structure):   # include/gsr_filter3d.h gsr_filter3d_camera; one row of the packed (C, 20) tensor
    _fields_ = [("R", ctypes.c_float * 9), ("t", ctypes.c_float * 3), ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float),
                ("cy", ctypes.c_float), ("W", ctypes.c_float), ("H", ctypes.c_float), ("pad", ctypes.c_float * 2)]


_i, _vp = ctypes.c_int, ctypes.c_void_p
_lib, _run = _binding.declare("gsr_filter3d.h", {
    "gsr_filter3d_scratch_bytes": (ctypes.c_size_t, [_i]),
    "gsr_filter3d_compute": (_i, [_i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "gsr_filter3d_activate": (_i, [_i] + [_vp] * 6),
    "gsr_filter3d_bake": (_i, [_i] + [_vp] * 6),
    "gsr_filter3d_activate_backward": (_i, [_i] + [_vp] * 8),
    "gsr_filter3d_reset_opacity": (_i, [_i, _vp, _vp, _vp, ctypes.c_double, _vp, _vp, _vp]),
}, {"gsr_filter3d_camera": FilterCamera})
_COLS = {"xyz": 3, "opacity": 1, "scaling": 3, "filter_3d": 1}
_check_device = functools.partial(_binding.check_device, "3D-filter kernels")


def _check(**named):
    """Every refusal of the tensors a call names (xyz (P,3), opacity (P,1), scaling (P,3), filter_3d (P,1)) but the device's, before the
    kernel library is touched.  -> P"""
    return _binding.check_rows([(n, t) for n, t in named.items() if n in _COLS], _COLS)


def _camera_scalars(cameras):
    """[(fx, fy, cx, cy, W, H)] of a list of camera objects; every refusal of the list, on the host"""
    if not isinstance(cameras, (list, tuple)) or len(cameras) < 1:
        raise TypeError("cameras must be a float32 (C, 20) tensor of packed records or a list of at least one camera")
    rows = []
    for n, cam in enumerate(cameras):
        W, H = int(cam.image_width), int(cam.image_height)
        model = _C.camera_model(getattr(cam, "camera_model", None))
        if model is None:   # the stock camera: focal lengths from the fields of view, centred
            rows.append((W / (2.0 * math.tan(0.5 * cam.FoVx)), H / (2.0 * math.tan(0.5 * cam.FoVy)), 0.5 * W, 0.5 * H, W, H))
        elif model.model == "pinhole":
            rows.append((model.fx, model.fy, model.cx, model.cy, W, H))
        else:
            raise NotImplementedError(f"camera {n}: the 3D filter's frustum test has no form for the {model.model!r} camera model")
        if not (W >= 1 and H >= 1 and all(math.isfinite(v) for v in rows[-1]) and rows[-1][0] > 0.0 and rows[-1][1] > 0.0):
            raise ValueError(f"camera {n}: focal lengths must be finite and positive, the image at least 1 x 1; got {rows[-1]}")
    return rows


def pack_cameras(cameras, device):
    """A list of camera objects -> the float32 (C, 20) tensor of gsr_filter3d_camera records on `device`: R[9] (row-major, p = R x + t),
    t[3], fx, fy, cx, cy, W, H and two pad words.  Read: `world_view_transform` in the reference's transposed convention
    (p = x @ wvt[:3,:3] + wvt[3,:3]), `FoVx`, `FoVy`, `image_width`, `image_height`; a pinhole `camera_model` attribute supplies
    fx, fy, cx, cy in place of the centred ones of the fields of view, a fisheye model raises NotImplementedError.  Pack once per
    training set: the records do not depend on the Gaussians."""
    rows = _camera_scalars(cameras)
    rec = torch.zeros((len(rows), CAMERA_FLOATS), dtype=torch.float32, device=device)
    wvt = torch.stack([torch.as_tensor(c.world_view_transform).detach().to(device=device, dtype=torch.float32) for c in cameras])
    if tuple(wvt.shape[1:]) != (4, 4):
        raise RuntimeError(f"world_view_transform must be (4, 4); got {tuple(wvt.shape[1:])}")
    rec[:, 0:9] = wvt[:, :3, :3].transpose(1, 2).reshape(-1, 9)
    rec[:, 9:12] = wvt[:, 3, :3]
    rec[:, 12:18] = torch.tensor(rows, dtype=torch.float64).to(device=device, dtype=torch.float32)
    return rec


@torch.no_grad()
def compute_filter_3d(xyz, cameras, per_camera=False):
    """Mip-Splatting's compute_3D_filter -> filter_3d (P, 1) float32.  Camera c sees Gaussian i where p = R_c x_i + t_c has p_z > 0.2 and
    its pixel lies within the image enlarged by 15 % on every side; d_i is the smallest p_z over the cameras that see it, a Gaussian
    no camera sees takes the largest d of those that are seen, and filter_3d = d / f_max * sqrt(0.2) with f_max the largest fx.
    per_camera=True uses the paper's own sampling rate, the smallest p_z / fx_c, which is the correct form where the cameras differ in
    resolution or focal length.  Where no camera sees any Gaussian the stock code raises; here every row holds 100000 (UNSEEN), which
    needs no read-back.
    xyz: (P, 3) float32 on the device (requires_grad and any strides are fine; no gradient flows).  cameras: the tensor pack_cameras()
    returns, or a list of camera objects, which is packed here on every call."""
    P = _check(xyz=xyz)
    if not isinstance(per_camera, bool):
        raise TypeError(f"per_camera must be True or False, got {per_camera!r}")
    if torch.is_tensor(cameras):
        if cameras.dim() != 2 or cameras.shape[0] < 1 or cameras.shape[1] != CAMERA_FLOATS or cameras.dtype != torch.float32:
            raise RuntimeError(f"cameras must be a float32 (C, {CAMERA_FLOATS}) tensor with C >= 1 (pack_cameras); got {cameras.dtype} "
                               f"{tuple(cameras.shape)}")
        dev = _check_device(xyz, cameras)
    else:
        _camera_scalars(cameras)
        dev = _check_device(xyz)
        cameras = pack_cameras(cameras, dev)
    lib = _lib()
    with torch.cuda.device(dev):
        x, cams = xyz.detach().contiguous(), cameras.contiguous()
        out = torch.empty((P, 1), dtype=torch.float32, device=dev)
        scratch = torch.empty(lib.gsr_filter3d_scratch_bytes(P), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        _run("gsr_filter3d_compute", P, int(cams.shape[0]), x.data_ptr(), cams.data_ptr(), int(per_camera), out.data_ptr(), scratch.data_ptr(),
             stream.cuda_stream)
        for t in (scratch, x, cams):
            t.record_stream(stream)
    return out


def _forward(entry, opacity, scaling, filter_3d, want):
    P = _check(opacity=opacity, scaling=scaling, filter_3d=filter_3d)
    for k in want:
        if k not in ("opacity", "scaling"):
            raise ValueError(f"want: unknown output {k!r}; the choices are ('opacity', 'scaling')")
    dev = _check_device(opacity, scaling, filter_3d)
    with torch.cuda.device(dev):
        l, ls, f = (t.detach().contiguous() for t in (opacity, scaling, filter_3d))
        out = {k: torch.empty_like(t) for k, t in (("opacity", l), ("scaling", ls)) if k in want}
        if out:
            _run(entry, P, l.data_ptr(), ls.data_ptr(), f.data_ptr(), ptr(out.get("opacity")), ptr(out.get("scaling")),
                 torch.cuda.current_stream(dev).cuda_stream)
    return out


@torch.no_grad()
def activate(opacity, scaling, filter_3d, want=("opacity", "scaling")):
    """-> {"opacity": opacities (P,1), "scaling": scales (P,3)}, raw and without autograd; only the outputs named in `want` are
    computed and written."""
    return _forward("gsr_filter3d_activate", opacity, scaling, filter_3d, want)


class _FilteredActivations(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opacity, scaling, filter_3d):
        out = _forward("gsr_filter3d_activate", opacity, scaling, filter_3d, ("opacity", "scaling"))
        ctx.save_for_backward(opacity, scaling, filter_3d)   # the backward recomputes the rest
        ctx.set_materialize_grads(False)                     # an absent upstream gradient stays absent: NULL for the kernel
        return out["opacity"], out["scaling"]

    @staticmethod
    def backward(ctx, g_opacities, g_scales):
        opacity, scaling, filter_3d = ctx.saved_tensors
        need_o, need_s = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (g_opacities is None and g_scales is None) or not (need_o or need_s):
            return None, None, None
        dev = opacity.device
        P = int(opacity.shape[0])
        with torch.cuda.device(dev):
            l, ls, f = (t.detach().contiguous() for t in (opacity, scaling, filter_3d))
            go = None if g_opacities is None else g_opacities.to(torch.float32).contiguous()
            gs = None if g_scales is None else g_scales.to(torch.float32).contiguous()
            d_o = torch.empty_like(l) if need_o else None
            d_s = torch.empty_like(ls) if need_s else None
            _run("gsr_filter3d_activate_backward", P, l.data_ptr(), ls.data_ptr(), f.data_ptr(), ptr(go), ptr(gs), ptr(d_o), ptr(d_s),
                 torch.cuda.current_stream(dev).cuda_stream)
        return d_o, d_s, None


def filtered_activations(opacity, scaling, filter_3d):
    """Mip-Splatting's get_opacity_with_3D_filter and get_scaling_with_3D_filter on the leaves -> (opacities (P,1), scales (P,3)):
    scales_k = sqrt(exp(scaling_k)^2 + f^2), opacities = sigmoid(opacity) * prod_k exp(scaling_k) / scales_k, differentiable w.r.t.
    opacity (P,1) logits and scaling (P,3) log-scales; filter_3d (P,1) is a buffer and gets no gradient.  The coefficient is formed per
    axis in double and rounded once: finite leaves and a positive filter give finite outputs and finite gradients that underflow
    smoothly, where the stock sqrt(det / det') underflows in fp32 and returns NaN gradients.  One launch forward, one backward; the
    backward recomputes the forward's values, so only the three inputs are kept."""
    _check(opacity=opacity, scaling=scaling, filter_3d=filter_3d)
    _check_device(opacity, scaling, filter_3d)
    return _FilteredActivations.apply(opacity, scaling, filter_3d)


@torch.no_grad()
def baked_leaves(opacity, scaling, filter_3d):
    """Mip-Splatting's save_fused_ply -> (logit(opacities) (P,1), log(scales) (P,3)) of filtered_activations(), formed in double and
    rounded once: the leaves a viewer that does not know the filter must load."""
    out = _forward("gsr_filter3d_bake", opacity, scaling, filter_3d, ("opacity", "scaling"))
    return out["opacity"], out["scaling"]


@torch.no_grad()
def reset_opacity(optimizer, filter_3d, max_opacity=0.01):
    """Mip-Splatting's reset_opacity: the filtered opacity sigmoid(l) coef is capped at max_opacity, that is
    l <- logit(min(sigmoid(l), max_opacity / coef)), in place on the optimizer's 'opacity' group with the coefficient of its 'scaling'
    group and filter_3d; both moments of the opacity group are zeroed.  A row at or below the cap keeps its bits; the others are
    evaluated in double and rounded once.  One launch.  fused_densify.reset_opacity is the reset without a filter.
    -> the opacity parameter"""
    from fused_mcmc import _leaf_groups
    if not 0.0 < float(max_opacity) < 1.0:
        raise ValueError(f"max_opacity must lie in (0, 1); got {max_opacity}")
    found = dict(_leaf_groups(optimizer))
    p, scaling = found["opacity"]["params"][0], found["scaling"]["params"][0]
    P = _check(opacity=p, scaling=scaling, filter_3d=filter_3d)
    state = optimizer.state.get(p, {})
    m, v = state.get("exp_avg"), state.get("exp_avg_sq")
    if (m is None) != (v is None):
        raise RuntimeError("the opacity group's exp_avg and exp_avg_sq go together")
    for n, t in (("opacity", p), ("exp_avg", m), ("exp_avg_sq", v)):
        if t is None:
            continue
        if t.dtype != torch.float32 or t.shape != p.shape:
            raise RuntimeError(f"{n} must be float32 and of shape {tuple(p.shape)}; got {t.dtype} {tuple(t.shape)}")
        if not t.is_contiguous():
            raise RuntimeError(f"{n} is changed in place and must be contiguous")
    dev = _check_device(*(t for t in (p, scaling, filter_3d, m, v) if t is not None))
    with torch.cuda.device(dev):
        ls, f = scaling.detach().contiguous(), filter_3d.detach().contiguous()
        _run("gsr_filter3d_reset_opacity", P, p.data_ptr(), ls.data_ptr(), f.data_ptr(), float(max_opacity), ptr(m), ptr(v),
             torch.cuda.current_stream(dev).cuda_stream)
    return p
