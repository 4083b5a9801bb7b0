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

from diff_gaussian_rasterization import _C, camera_grad_results, camera_inputs, camera_model_grad_results

_vp, _i64, _d = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
ADAM_MAX_GROUPS = 8


class AdamGroup(ctypes.Structure):
    """include/gsr.h gsr_adam_group"""
    _fields_ = [("param", _vp), ("grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("numel", _i64), ("step", _i64),
                ("lr", _d), ("row", ctypes.c_int32)]


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
    """(xyz, means2D, _features_dc, _features_rest, _opacity, _scaling, _rotation) -> (color, radii); the same
    contract as diff_gaussian_rasterization._RasterizeGaussians with the activations folded in, its depth and alpha maps included:
    with depth_alpha -> (color, radii, depth (1,H,W), alpha (1,H,W)); without gradients for either map the default backward kernels run.
    `stats` (optional): (xyz_gradient_accum, denom, max_radii2D) float32 [P] tensors updated in place by the
    backward for the Gaussians visible in this view (train.py:157-159, gaussian_model.py:599-602)."""

    @staticmethod
    def forward(ctx, xyz, means2D, features_dc, features_rest, opacity, scaling, rotation, raster_settings, stats=None,
                depth_alpha=None, antialiasing=False, contrib_stats=None, contrib_pixel_weight=None, absgrad=None, *camera,
                _features=None, _distortion=False, _median=False, _index_maps=None, _lead=None):
        _C.distortion_flag(_distortion, depth_alpha)   # refused before anything runs
        _C.median_flag(_median, depth_alpha)           # the same
        if _index_maps is not None:   # the same
            _C.index_map_tensors(_index_maps, raster_settings.image_width, raster_settings.image_height,
                                 xyz.device if xyz.is_cuda else None)
        if _features is not None:       # the same
            _C.feature_tensor(_features, int(xyz.size(0)), xyz.device if xyz.is_cuda else None)
        if contrib_stats is not None:   # the same
            _C.contrib_stat_tensors(contrib_stats, int(xyz.size(0)))
        if absgrad is not None:         # the same; only the backward writes the tensors (GaussianRasterizer, absgrad)
            _C.absgrad_tensors(absgrad, int(xyz.size(0)), xyz.device if xyz.is_cuda else None)
        R, color, radii, geom, binning, img, M, (xyz, features_dc, features_rest, scaling, rotation), *maps = _leaf_forward(
            None if depth_alpha is None else _C.aux_mode(depth_alpha), xyz, features_dc, features_rest, opacity, scaling, rotation,
            raster_settings, antialiasing, camera[0] if len(camera) in (1, 4) else None)
        if len(camera) == 4 and camera[3] is not None and raster_settings.debug:   # the handle of the intrinsics and the model agree
            _C.camera_model_matches(_C.camera_model(camera[0]), camera[3])
        if contrib_stats is not None:   # the blend-weight statistics of this view (GaussianRasterizer): once per forward, never in backward
            _C.gaussian_contributions(geom, binning, img, R, int(xyz.size(0)), raster_settings.image_width, raster_settings.image_height,
                                      contrib_stats, contrib_pixel_weight, raster_settings.debug)
        ctx.raster_settings, ctx.num_rendered, ctx.M, ctx.stats, ctx.depth_alpha = raster_settings, R, M, stats, depth_alpha
        fmap = ()
        if _features is not None:   # the feature map of GaussianRasterizer (features=), from the state the render just left
            fmap = (_C.features_forward(geom, binning, img, R, int(xyz.size(0)), raster_settings.image_width,
                                        raster_settings.image_height, _features, raster_settings.debug),)
        dmap = dstate = ()
        if _distortion:   # the distortion map of GaussianRasterizer (distortion=True), from the same state
            d, dst = _C.distortion_forward(geom, binning, img, R, int(xyz.size(0)), raster_settings.image_width,
                                           raster_settings.image_height, raster_settings.debug)
            dmap, dstate = (d,), (dst,)
        mmap = mstate = ()
        if _median or _index_maps is not None:   # the median-depth map and / or the index maps of GaussianRasterizer: one launch
            md, mst = _C.median_forward(geom, binning, img, R, int(xyz.size(0)), raster_settings.image_width,
                                        raster_settings.image_height, _index_maps, _median, raster_settings.debug)
            if _median:
                mmap, mstate = (md,), (mst,)
        ctx.features = _features is not None   # then input 0 is `features` and every other input sits one place further back
        ctx.distortion = _distortion           # then input 0 is `features` too, a tensor or None
        ctx.median = _median
        # how many inputs of the applied Function sit in front of this class's own
        ctx.lead = _lead if _lead is not None else (1 if (_features is not None or _distortion) else 0)
        ctx.antialiasing = antialiasing
        ctx.absgrad = absgrad
        ctx.camera = len(camera) == 3   # the settings' viewmatrix, projmatrix, campos as inputs (GaussianRasterizer, camera_grads)
        ctx.camera_model = camera[0] if len(camera) in (1, 4) else None   # or the one checked CameraModel (GaussianRasterizer, camera_model)
        ctx.camera_cm = len(camera) == 4   # ... with the settings' viewmatrix, campos and the intrinsics tensor (or None) behind it (camera_model_grads)
        # after the state: the aux state of the maps, the distortion map's and the median depth's per-pixel state, and the opacity logits
        # that the anti-aliased backward reads (the records hold sigmoid(logit) * rho), each saved on its path only
        ctx.save_for_backward(xyz, features_dc, features_rest, scaling, rotation, radii, geom, binning, img,
                              *(() if _features is None else (_features,)), *maps[2:], *dstate, *mstate,
                              *((opacity,) if antialiasing else ()))
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)   # no zero tensor for the radii output on the way back
        return (color, radii, *maps[:2], *dmap, *mmap, *fmap)

    @staticmethod
    def backward(ctx, grad_color, _, grad_depth=None, grad_alpha=None):
        return _RasterizeLeafGaussians.backward_with(ctx, grad_color, grad_depth, grad_alpha, None)[1]

    @staticmethod
    def backward_with(ctx, grad_color, grad_depth, grad_alpha, grad_features_map, grad_distortion=None, grad_median=None):
        """-> (dL/dfeatures or None, the gradient tuple of this class's inputs)"""
        st, R, M = ctx.raster_settings, ctx.num_rendered, ctx.M
        xyz, features_dc, features_rest, scaling, rotation, radii, geom, binning, img, *extra = ctx.saved_tensors
        dev = xyz.device
        off = ctx.lead
        fb = None
        if ctx.features:
            features, extra = extra[0], extra[1:]
            if grad_features_map is not None and ctx.needs_input_grad[0] and not any(ctx.needs_input_grad[1:]):
                # features on a frozen scene: their gradient alone, no colour backward, no gradient slots
                return (_C.features_backward_only(geom, binning, img, R, int(xyz.size(0)), st.image_width, st.image_height, features,
                                                  grad_features_map, st.debug),
                        (None,) * (14 + (3 if ctx.camera else 0) + (1 if ctx.camera_model is not None else 0) + (3 if ctx.camera_cm else 0)))
            if grad_features_map is not None:   # (no gradient reached the map: the feature pass is skipped)
                fb = _C.FeatureBackward(features, grad_features_map)
        if grad_color is None:
            grad_color = torch.zeros((3, int(st.image_height), int(st.image_width)), dtype=torch.float32, device=dev)
        P = int(xyz.size(0))
        f32 = dict(dtype=torch.float32, device=dev)
        cam_needs = tuple(ctx.needs_input_grad[14 + off:17 + off]) if ctx.camera else ()
        cam, cam_grads = None, (None, None, None) if ctx.camera else ()
        cm_needs = tuple(ctx.needs_input_grad[15 + off:18 + off]) if ctx.camera_cm else ()
        cm_grads = (None, None, None) if ctx.camera_cm else ()
        with torch.cuda.device(dev):
            alloc = torch.zeros if P == 0 else torch.empty
            d_means2D, d_xyz = alloc((P, 3), **f32), alloc((P, 3), **f32)
            d_dc, d_rest = alloc((P, 1, 3), **f32), alloc((P, M - 1, 3), **f32)
            d_opacity, d_scaling, d_rotation = alloc((P, 1), **f32), alloc((P, 3), **f32), alloc((P, 4), **f32)
            if P:
                grad_color = _C._dev_f32(grad_color, dev, "dL_dout_color")
                scratch = _C.backward_scratch(P, R, dev)
                a = leaf_backward_args(st, R, M, xyz, features_dc, features_rest, scaling, rotation, radii, geom, binning, img,
                                       scratch, grad_color)
                _C.set_backward_outputs(a, dL_dmean2D=d_means2D, dL_dmean3D=d_xyz, dL_dsh=d_dc, dL_dsh_rest=d_rest,
                                        dL_dopacity=d_opacity, dL_dscale=d_scaling, dL_drot=d_rotation)
                _C.set_backward_stats(a, ctx.stats, P, dev)
                x = db = mb = None
                if ctx.median and grad_median is not None:   # the same for the median depth; its state sits behind the distortion state
                    mb = _C.MedianBackward(extra[2 if ctx.distortion else 1], grad_median)
                if ctx.distortion and grad_distortion is not None:   # (no gradient reached the map: nothing of it runs)
                    db = _C.DistortionBackward(extra[1], grad_distortion)
                if grad_depth is not None or grad_alpha is not None or db is not None or mb is not None:
                    # (the distortion map's or the median depth's gradient alone still takes the aux kernels: they write the slots' dL/dv
                    # word and chain it)
                    hw = lambda g: None if g is None else g.reshape(g.shape[-2:])
                    x = _C.aux_backward_args(ctx.depth_alpha, extra[0], hw(grad_depth), hw(grad_alpha), dev)
                if any(cam_needs):
                    cam, outs = _C.camera_backward_args(P, dev)
                elif any(cm_needs):   # the camera gradients under the model (include/gsr_cam_cm.h)
                    cam, outs = _C.camera_cm_backward_args(P, dev)
                _C.run_backward(a, scratch, dev, x, extra[-1] if ctx.antialiasing else None, cam=cam,
                                absgrad=None if ctx.absgrad is None else _C.absgrad_tensors(ctx.absgrad, P, dev), features=fb,
                                distortion=db, median=mb, camera_model=ctx.camera_model)
            elif any(cam_needs):
                outs = (torch.zeros((4, 4), **f32), torch.zeros((4, 4), **f32), torch.zeros((3,), **f32))
            elif any(cm_needs):
                outs = (torch.zeros((4, 4), **f32), torch.zeros((4,), **f32), torch.zeros((3,), **f32))
            if any(cam_needs):
                cam_grads = camera_grad_results(cam_needs, outs, (st.viewmatrix, st.projmatrix, st.campos))
            if any(cm_needs):
                cm_grads = camera_model_grad_results(cm_needs, outs, st)
        grad_features = None
        if fb is not None:   # (no Gaussian: nothing ran)
            grad_features = fb.grad if fb.grad is not None else torch.zeros_like(fb.features)
        return grad_features, (d_xyz, d_means2D, d_dc, d_rest, d_opacity, d_scaling, d_rotation, None, None, None, None, None, None, None,
                               *cam_grads, *((None,) if ctx.camera_model is not None else ()), *cm_grads)


class _RasterizeLeafGaussiansFeatures(torch.autograd.Function):
    """_RasterizeLeafGaussians with `features` (P, K) in front of its inputs -> (color, radii[, depth, alpha], feature_map (K, H, W)),
    the counterpart of diff_gaussian_rasterization._RasterizeGaussiansFeatures."""

    @staticmethod
    def forward(ctx, features, *inputs):
        return _RasterizeLeafGaussians.forward(ctx, *inputs, _features=features)

    @staticmethod
    def backward(ctx, grad_color, _, *grads):
        grad_depth, grad_alpha = grads[:2] if len(grads) == 3 else (None, None)
        grad_features, rest = _RasterizeLeafGaussians.backward_with(ctx, grad_color, grad_depth, grad_alpha, grads[-1])
        return (grad_features, *rest)


class _RasterizeLeafGaussiansDistortion(torch.autograd.Function):
    """_RasterizeLeafGaussians with a depth_alpha mode and the distortion map -> (color, radii, depth, alpha, distortion (1, H, W)
    [, feature_map]), `features` (P, K) or None in front of its inputs: the counterpart of
    diff_gaussian_rasterization._RasterizeGaussiansDistortion."""

    @staticmethod
    def forward(ctx, features, *inputs):
        return _RasterizeLeafGaussians.forward(ctx, *inputs, _features=features, _distortion=True)

    @staticmethod
    def backward(ctx, grad_color, _, grad_depth, grad_alpha, grad_distortion, *grad_fmap):
        grad_features, rest = _RasterizeLeafGaussians.backward_with(ctx, grad_color, grad_depth, grad_alpha,
                                                                    grad_fmap[0] if grad_fmap else None, grad_distortion)
        return (grad_features, *rest)


class _RasterizeLeafGaussiansMedian(torch.autograd.Function):
    """_RasterizeLeafGaussians with the median-depth map and / or the per-pixel index maps; `features` or None, the distortion and
    median_depth flags and index_maps in front of its inputs: the counterpart of diff_gaussian_rasterization._RasterizeGaussiansMedian."""

    @staticmethod
    def forward(ctx, features, distortion, median_depth, index_maps, *inputs):
        return _RasterizeLeafGaussians.forward(ctx, *inputs, _features=features, _distortion=distortion, _median=median_depth,
                                               _index_maps=index_maps, _lead=4)

    @staticmethod
    def backward(ctx, grad_color, _, *grads):
        g = list(grads)
        grad_depth, grad_alpha = (g.pop(0), g.pop(0)) if ctx.depth_alpha is not None else (None, None)
        grad_distortion = g.pop(0) if ctx.distortion else None
        grad_median = g.pop(0) if ctx.median else None
        grad_features, rest = _RasterizeLeafGaussians.backward_with(ctx, grad_color, grad_depth, grad_alpha, g[0] if g else None,
                                                                    grad_distortion, grad_median)
        return (grad_features, None, None, None, *rest)


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
    if depth_alpha is not None:
        _C.aux_mode(depth_alpha)
    distortion = _C.distortion_flag(distortion, depth_alpha)
    median_depth = _C.median_flag(median_depth, depth_alpha)
    if index_maps is not None:
        _C.index_map_tensors(index_maps, raster_settings.image_width, raster_settings.image_height)
    inputs = (xyz, means2D, features_dc, features_rest, opacity, scaling, rotation, raster_settings, stats, depth_alpha,
              _C.aa_flag(antialiasing), contrib_stats, contrib_pixel_weight, absgrad,
              *camera_inputs(raster_settings, camera_grads, camera_model, camera_model_grads))
    if features is not None:
        _C.feature_tensor(features, int(xyz.size(0)))   # refused before anything runs
    if median_depth or index_maps is not None:
        return _RasterizeLeafGaussiansMedian.apply(features, distortion, median_depth, index_maps, *inputs)
    if distortion:
        return _RasterizeLeafGaussiansDistortion.apply(features, *inputs)
    if features is None:
        return _RasterizeLeafGaussians.apply(*inputs)
    return _RasterizeLeafGaussiansFeatures.apply(features, *inputs)


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam (no weight decay / amsgrad / maximize) whose step() is one HIP kernel over all groups.

    Built like the reference builds its optimiser: `FusedAdam(l, lr=0.0, eps=1e-15)` with
    `l = [{'params': [t], 'lr': ..., 'name': ...}, ...]` (gaussian_model.py:243-252).
    `step(visible_radii=radii)` is the opt-in visible-only variant (NOT the reference's update rule):
    Gaussians with radii <= 0 keep parameters and moments untouched; it needs every tensor's dim 0 = P."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))

    @torch.no_grad()
    def step(self, closure=None, visible_radii=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        batches = {}  # (device, betas, eps) -> [AdamGroup]
        keep = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("FusedAdam needs contiguous float32 HIP (cuda) parameters; there is no CPU path")
                if p.grad.is_sparse:
                    raise RuntimeError("FusedAdam does not support sparse gradients")
                state = self.state[p]
                if len(state) == 0 or "exp_avg" not in state:
                    state["step"] = state.get("step", 0)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                step = int(state["step"]) + 1  # an int or a 0-dim tensor (states edited by densification code)
                state["step"] = step
                g = p.grad.contiguous()
                m, v = state["exp_avg"], state["exp_avg_sq"]
                if not (m.is_contiguous() and v.is_contiguous()):
                    raise RuntimeError("FusedAdam: optimizer state tensors must be contiguous")
                keep.append(g)
                row = p.numel() // p.size(0) if (p.dim() > 0 and p.size(0) > 0) else 1
                key = (p.device, tuple(float(b) for b in group["betas"]), float(group["eps"]))
                batches.setdefault(key, []).append(AdamGroup(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), step,
                                                             float(group["lr"]), row))
        L = _C.lib()
        for (dev, betas, eps), groups in batches.items():
            radii_ptr = None
            if visible_radii is not None:
                if visible_radii.dtype != torch.int32 or visible_radii.device != dev or not visible_radii.is_contiguous():
                    raise RuntimeError("visible_radii must be a contiguous int32 tensor on the parameters' device")
                radii_ptr = visible_radii.data_ptr()
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                for k in range(0, len(groups), ADAM_MAX_GROUPS):
                    chunk = groups[k:k + ADAM_MAX_GROUPS]
                    arr = (AdamGroup * len(chunk))(*chunk)
                    _C._check(L.gsr_adam_step(len(chunk), arr, betas[0], betas[1], eps, radii_ptr, stream))
        return loss
