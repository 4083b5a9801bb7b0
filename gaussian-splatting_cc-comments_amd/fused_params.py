"""Leaf-parameter rasterization and fused Adam.

The reference renders from ACTIVATED copies of its optimiser leaves -- `pc.get_scaling = exp(_scaling)`,
`pc.get_rotation = normalize(_rotation)`, `pc.get_opacity = sigmoid(_opacity)`, `pc.get_features =
cat(_features_dc, _features_rest)` (scene/gaussian_model.py:114-135, gaussian_renderer/__init__.py:59-86)
-- and autograd walks those four ops back after the rasterizer's backward: ~0.9 KB of HBM traffic per
Gaussian per step around a rasterizer that itself moves ~1.3 KB per Gaussian.  Here the per-Gaussian
kernels read the leaves directly and write gradients w.r.t. the leaves (include/gsr.h
gsr_forward_preprocess_leaf / gsr_backward_leaf); no activated tensor is ever materialised.

`FusedAdam` is torch.optim.Adam as gaussian_model.py:243-252 configures it (eps 1e-15, per-group lr,
one tensor per group) with `step()` done by ONE kernel over all groups (include/gsr.h gsr_adam_step).
It keeps torch.optim.Adam's state layout (`state[p] = {"step", "exp_avg", "exp_avg_sq"}`), so the
reference's densification code that edits the optimiser state (gaussian_model.py:412-460) works on it
unchanged.  HIP tensors only -- no CPU fallback.
"""
import ctypes

import torch

from diff_gaussian_rasterization import OPTION_INPUTS, _binding, _C, after_backward, after_render, before_backward, camera_positions

_vp, _i64, _d = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
ADAM_MAX_GROUPS = 8


class AdamGroup(ctypes.Structure):
    """include/gsr.h gsr_adam_group"""
    _fields_ = [("param", _vp), ("grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("numel", _i64), ("step", _i64),
                ("lr", _d), ("row", ctypes.c_int32)]


_binding.declare("gsr.h", {}, {"gsr_adam_group": AdamGroup})   # the mirror alone: _C declares gsr_adam_step with the rest of gsr.h

def _leaf_forward(mode, xyz, features_dc, features_rest, opacity, scaling, rotation, raster_settings, antialiasing, camera_model=None):
    st = raster_settings
    P = int(xyz.size(0))
    M = 1 + (int(features_rest.size(1)) if features_rest.numel() else 0)
    if features_dc.shape != (P, 1, 3) or (M > 1 and features_rest.shape != (P, M - 1, 3)):
        raise RuntimeError(f"features_dc must be (P,1,3) and features_rest (P,M-1,3); got {tuple(features_dc.shape)}, "
                           f"{tuple(features_rest.shape)}")
    R, color, radii, geom, binning, img, (xyz, features_dc, features_rest, _, scaling, rotation, *_), maps = _C.run_forward(
        True, mode, antialiasing, st.bg,
        ((xyz, "xyz"), (features_dc, "features_dc"), (features_rest, "features_rest"), (opacity, "opacity"), (scaling, "scaling"),
         (rotation, "rotation"), (st.viewmatrix, "viewmatrix"), (st.projmatrix, "projmatrix"), (st.campos, "campos")),
        st.sh_degree, M, st.image_width, st.image_height, st.scale_modifier, st.tanfovx, st.tanfovy, st.prefiltered, st.debug,
        _C.camera_model(camera_model))
    return (R, color, radii, geom, binning, img, M, (xyz, features_dc, features_rest, scaling, rotation), *maps)


def leaf_forward(xyz, features_dc, features_rest, opacity, scaling, rotation, raster_settings, antialiasing=False):
    """Forward from the raw leaves -> (num_rendered, color, radii, geom, binning, img, M, contiguous inputs).
    antialiasing: the screen-space filter (include/gsr_aa.h)."""
    return _leaf_forward(None, xyz, features_dc, features_rest, opacity, scaling, rotation, raster_settings, antialiasing)


def leaf_forward_depth_alpha(depth_alpha, xyz, features_dc, features_rest, opacity, scaling, rotation, raster_settings,
                             antialiasing=False):
    """leaf_forward() with the depth and alpha maps (include/gsr_aux.h) -> (num_rendered, color, radii, geom, binning,
    img, M, contiguous inputs, depth (1,H,W), alpha (1,H,W), aux scratch)."""
    return _leaf_forward(_C.aux_mode(depth_alpha), xyz, features_dc, features_rest, opacity, scaling, rotation, raster_settings,
                         antialiasing)


def leaf_backward_args(st, R, M, xyz, features_dc, features_rest, scaling, rotation, radii, geom, binning, img, scratch, grad_color):
    """gsr_backward_args (leaf = 1) for a state produced by leaf_forward(); gradient pointers still unset."""
    dev = xyz.device
    bg, view, proj, campos = (_C._dev_f32(t, dev, n) for t, n in ((st.bg, "bg"), (st.viewmatrix, "viewmatrix"),
                                                                  (st.projmatrix, "projmatrix"), (st.campos, "campos")))
    a = _C.backward_args(P=int(xyz.size(0)), D=int(st.sh_degree), M=M, R=R, W=int(st.image_width), H=int(st.image_height), leaf=1,
                         background=bg, means3D=xyz, shs=features_dc, shs_rest=features_rest, scales=scaling,
                         scale_modifier=st.scale_modifier, rotations=rotation, viewmatrix=view, projmatrix=proj, cam_pos=campos,
                         tan_fovx=st.tanfovx, tan_fovy=st.tanfovy, radii=radii, geometry=geom, binning=binning, image=img,
                         scratch=scratch, dL_dpix=grad_color, debug=st.debug, device=dev)
    a._keep = (bg, view, proj, campos)  # alive as long as the struct
    return a


class _RasterizeLeafGaussians(torch.autograd.Function):
    """(xyz, means2D, _features_dc, _features_rest, _opacity, _scaling, _rotation, raster_settings) and then the OPTION_INPUTS of
    diff_gaussian_rasterization._RasterizeGaussians -> (color, radii[, depth, alpha][, distortion][, median_depth][, feature_map]):
    the same contract with the activations folded in, and the same shared steps around the render and the backward (after_render(),
    before_backward(), after_backward()).  What differs is here: the leaf forward, leaf_backward_args() and the gradients w.r.t. the
    leaves.  options.densify_stats: (xyz_gradient_accum, denom, max_radii2D) float32 [P] tensors updated in place by the backward
    for the Gaussians visible in this view (train.py:157-159, gaussian_model.py:599-602)."""

    INPUTS = ("xyz", "means2D", "features_dc", "features_rest", "opacity", "scaling", "rotation", "raster_settings") + OPTION_INPUTS

    @staticmethod
    def forward(ctx, xyz, means2D, features_dc, features_rest, opacity, scaling, rotation, raster_settings, options=None,
                features=None, viewmatrix=None, projmatrix=None, campos=None, intrinsics=None):
        options = _C.RenderOptions() if options is None else options
        P = int(xyz.size(0))
        # refused before anything runs
        _C.check_render_tensors(options, features, intrinsics, P, xyz.device if xyz.is_cuda else None, raster_settings)
        R, color, radii, geom, binning, img, M, (xyz, features_dc, features_rest, scaling, rotation), *maps = _leaf_forward(
            None if options.depth_alpha is None else _C.aux_mode(options.depth_alpha), xyz, features_dc, features_rest, opacity,
            scaling, rotation, raster_settings, options.antialiasing, options.camera_model)
        ctx.M = M
        state = dict(means3D=xyz, features_dc=features_dc, features_rest=features_rest, scaling=scaling, rotation=rotation, radii=radii,
                     geomBuffer=geom, binningBuffer=binning, imgBuffer=img)
        # (the opacity logits for the anti-aliased backward: the records hold sigmoid(logit) * rho)
        return after_render(ctx, options, features, raster_settings, P, R, color, radii, maps, state, opacity)

    @staticmethod
    def backward(ctx, *grad_outputs):
        plan = before_backward(ctx, _RasterizeLeafGaussians.INPUTS, grad_outputs)
        if plan.answer is not None:
            return tuple(map(plan.answer.get, _RasterizeLeafGaussians.INPUTS))
        st, R, M, P, options, s = ctx.raster_settings, ctx.num_rendered, ctx.M, ctx.P, ctx.options, plan.saved
        xyz, radii = s["means3D"], s["radii"]
        dev = xyz.device
        f32 = dict(dtype=torch.float32, device=dev)
        cam = camera_grads = None
        with torch.cuda.device(dev):
            alloc = torch.zeros if P == 0 else torch.empty
            d_means2D, d_xyz = alloc((P, 3), **f32), alloc((P, 3), **f32)
            d_dc, d_rest = alloc((P, 1, 3), **f32), alloc((P, M - 1, 3), **f32)
            d_opacity, d_scaling, d_rotation = alloc((P, 1), **f32), alloc((P, 3), **f32), alloc((P, 4), **f32)
            if plan.camera is not None:   # (no Gaussian: no struct, zeros)
                cam, camera_grads = _C.camera_target(plan.camera, P, dev)
            if P:
                grad_color = _C._dev_f32(plan.grad_color, dev, "dL_dout_color")
                scratch = _C.backward_scratch(P, R, dev)
                a = leaf_backward_args(st, R, M, xyz, s["features_dc"], s["features_rest"], s["scaling"], s["rotation"], radii,
                                       s["geomBuffer"], s["binningBuffer"], s["imgBuffer"], scratch, grad_color)
                _C.set_backward_outputs(a, dL_dmean2D=d_means2D, dL_dmean3D=d_xyz, dL_dsh=d_dc, dL_dsh_rest=d_rest,
                                        dL_dopacity=d_opacity, dL_dscale=d_scaling, dL_drot=d_rotation)
                _C.set_backward_stats(a, options.densify_stats, P, dev)
                x = _C.aux_backward_args(options.depth_alpha, s["aux_state"], *plan.map_grads, dev) if plan.aux else None
                _C.run_backward(a, scratch, dev, x, s["opacities"] if options.antialiasing else None, cam=cam,
                                absgrad=None if options.absgrad is None else _C.absgrad_tensors(options.absgrad, P, dev),
                                features=plan.features, distortion=plan.distortion, median=plan.median,
                                camera_model=options.camera_model)
        out = after_backward(plan, camera_grads, st)
        out.update(xyz=d_xyz, means2D=d_means2D, features_dc=d_dc, features_rest=d_rest, opacity=d_opacity, scaling=d_scaling,
                   rotation=d_rotation)
        return tuple(map(out.get, _RasterizeLeafGaussians.INPUTS))   # everything not named: None


def rasterize_leaf_gaussians(xyz, means2D, features_dc, features_rest, opacity, scaling, rotation, raster_settings, stats=None,
                             depth_alpha=None, antialiasing=False, contrib_stats=None, contrib_pixel_weight=None, camera_grads=False,
                             absgrad=None, features=None, distortion=False, median_depth=False, index_maps=None, camera_model=None,
                             camera_model_grads=False):
    """Equivalent to
        GaussianRasterizer(raster_settings)(means3D=xyz, means2D=means2D, shs=cat(features_dc, features_rest, 1),
            opacities=sigmoid(opacity), scales=exp(scaling), rotations=normalize(rotation))
    -> (color (3,H,W), radii (P,) int32); with depth_alpha = "depth" / "invdepth" -> (color, radii, depth, alpha), the maps of
    GaussianRasterizer(raster_settings, depth_alpha=...).  antialiasing: the screen-space filter of
    GaussianRasterizer(raster_settings, antialiasing=True); the opacity gradient is w.r.t. the logits as always.
    stats: GaussianRasterizer's densify_stats, updated by the backward.
    contrib_stats / contrib_pixel_weight: the blend-weight statistics of GaussianRasterizer, updated by the forward.
    camera_grads: the settings' viewmatrix, projmatrix and campos take part in autograd, as in GaussianRasterizer.
    absgrad: (abs_mean2D, abs_gradient_accum), the absolute screen-space gradients of GaussianRasterizer, written by the backward.
    features: (P, K) float32 feature channels; the tuple then ends with feature_map (K, H, W), as GaussianRasterizer's (features=):
    differentiable w.r.t. features and, through the colour backward's slots, w.r.t. the leaves.
    distortion: True (with depth_alpha) puts the depth-distortion map (1, H, W) behind depth and alpha, as GaussianRasterizer's
    (distortion=True): differentiable w.r.t. the leaves, xyz's depth included.
    median_depth: True (with depth_alpha) puts the median-depth map (1, H, W) behind alpha (and distortion), in front of the feature
    map, as GaussianRasterizer's (median_depth=True): differentiable w.r.t. xyz along the view z axis.
    index_maps: (median_index, dominant_index, dominant_weight), overwritten in place by the forward, as GaussianRasterizer's.
    camera_model: a CameraModel ("pinhole" with intrinsics or "fisheye"), as GaussianRasterizer's: the settings' projmatrix, tanfovx and
    tanfovy are then ignored; not with camera_grads (NotImplementedError): camera_model_grads is its form for a model.
    camera_model_grads: True or the float32 (4,) intrinsics tensor (with camera_model), as GaussianRasterizer's: the settings'
    viewmatrix and campos, and the tensor, take part in autograd behind the model."""
    options, intrinsics = _C.render_options(raster_settings, depth_alpha, stats, antialiasing, contrib_stats, contrib_pixel_weight,
                                            camera_grads, absgrad, distortion, median_depth, index_maps, camera_model,
                                            camera_model_grads)
    return _RasterizeLeafGaussians.apply(xyz, means2D, features_dc, features_rest, opacity, scaling, rotation, raster_settings,
                                         options, features, *camera_positions(options, raster_settings, intrinsics))


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam (no weight decay / amsgrad / maximize) whose step() is one HIP kernel over all groups.

    Built like the reference builds its optimiser: `FusedAdam(l, lr=0.0, eps=1e-15)` with
    `l = [{'params': [t], 'lr': ..., 'name': ...}, ...]` (gaussian_model.py:243-252).
    `step(visible_radii=radii)` is the opt-in visible-only variant (NOT the reference's update rule):
    Gaussians with radii <= 0 keep parameters and moments untouched.  The kernel reads radii[row] for every
    row of every tensor, so every parameter that has a gradient must have radii.numel() rows (dim 0 = P);
    a step that cannot be taken is refused before any state is touched."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))

    def _check_step(self, visible_radii):
        """Every refusal of step(), before a step count, a moment or a parameter is touched."""
        if visible_radii is not None:
            if not torch.is_tensor(visible_radii) or visible_radii.dim() != 1 or visible_radii.dtype != torch.int32 or \
                    not visible_radii.is_cuda or not visible_radii.is_contiguous():
                raise RuntimeError("FusedAdam: visible_radii must be a contiguous 1-D int32 tensor on the parameters' device")
        for k, group in enumerate(self.param_groups):
            name = f"group {group.get('name', k)!r}"
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError(f"FusedAdam, {name}: needs contiguous float32 HIP (cuda) parameters; there is no CPU path")
                if p.grad.is_sparse:
                    raise RuntimeError(f"FusedAdam, {name}: does not support sparse gradients")
                if p.grad.dtype != torch.float32 or p.grad.device != p.device or p.grad.shape != p.shape:
                    raise RuntimeError(f"FusedAdam, {name}: the gradient must be float32, on the parameter's device and of its shape")
                state = self.state.get(p, {})
                for key in ("exp_avg", "exp_avg_sq"):
                    t = state.get(key)
                    if t is None:
                        continue
                    if not t.is_contiguous():
                        raise RuntimeError(f"FusedAdam, {name}: optimizer state tensors must be contiguous")
                    if t.dtype != torch.float32 or t.device != p.device or t.shape != p.shape:
                        raise RuntimeError(f"FusedAdam, {name}: {key} must be float32, on the parameter's device and of its shape "
                                           f"{tuple(p.shape)}; got {t.dtype} {tuple(t.shape)} on {t.device}")
                if ("exp_avg" in state) != ("exp_avg_sq" in state):
                    raise RuntimeError(f"FusedAdam, {name}: exp_avg and exp_avg_sq go together")
                if visible_radii is not None:
                    if visible_radii.device != p.device:
                        raise RuntimeError(f"FusedAdam, {name}: visible_radii is on {visible_radii.device}, the parameter on {p.device}")
                    if p.dim() < 1 or p.size(0) != visible_radii.numel():
                        raise RuntimeError(f"FusedAdam, {name}: visible_radii has {visible_radii.numel()} rows, the parameter has shape "
                                           f"{tuple(p.shape)}: with visible_radii every parameter needs dim 0 = P")

    @torch.no_grad()
    def step(self, closure=None, visible_radii=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_step(visible_radii)
        batches = {}  # (device, betas, eps) -> [AdamGroup]
        keep = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if len(state) == 0 or "exp_avg" not in state:
                    state["step"] = state.get("step", 0)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                step = int(state["step"]) + 1  # an int or a 0-dim tensor (states edited by densification code)
                state["step"] = step
                g = p.grad.contiguous()
                m, v = state["exp_avg"], state["exp_avg_sq"]
                keep.append(g)
                row = max(1, p.numel() // p.size(0)) if (p.dim() > 0 and p.size(0) > 0) else 1   # (P, 0, 3): no element, row 1
                key = (p.device, tuple(float(b) for b in group["betas"]), float(group["eps"]))
                batches.setdefault(key, []).append(AdamGroup(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), step,
                                                             float(group["lr"]), row))
        L = _C.lib()
        for (dev, betas, eps), groups in batches.items():
            radii_ptr = None if visible_radii is None else visible_radii.data_ptr()
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                for k in range(0, len(groups), ADAM_MAX_GROUPS):
                    chunk = groups[k:k + ADAM_MAX_GROUPS]
                    arr = (AdamGroup * len(chunk))(*chunk)
                    _C._check(L.gsr_adam_step(len(chunk), arr, betas[0], betas[1], eps, radii_ptr, stream))
        return loss
