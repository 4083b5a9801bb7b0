"""Drop-in replacement for the reference's `diff_gaussian_rasterization` package
(submodules/diff-gaussian-rasterization/diff_gaussian_rasterization/__init__.py): same names,
signatures, validation errors, saved-tensor set, gradient order and debug snapshot behaviour.
The only difference is underneath: `_C` is a ctypes binding of the gfx950 C-ABI library
(include/gsr.h) instead of a CUDA torch extension.

    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
"""
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _C


def cpu_deep_copy_tuple(input_tuple):
    """reference __init__.py:17-19"""
    copied_tensors = [item.cpu().clone() if isinstance(item, torch.Tensor) else item for item in input_tuple]
    return tuple(copied_tensors)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, densify_stats=None, antialiasing=False, contrib_stats=None, contrib_pixel_weight=None,
                        camera_grads=False, absgrad=None, features=None, index_maps=None, camera_model=None,
                        camera_model_grads=False):
    """reference __init__.py:22-45 (+ the optional densification-statistics tensors, the screen-space filter, the blend-weight
    statistics, the camera gradients, the absolute gradients, the feature channels, the per-pixel index maps, the camera model and
    the camera gradients under it, see GaussianRasterizer)"""
    if index_maps is not None:
        _C.index_map_tensors(index_maps, raster_settings.image_width, raster_settings.image_height)
    return _apply(features, means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                  cov3Ds_precomp, raster_settings, densify_stats, _C.aa_flag(antialiasing), None,
                  contrib_stats, contrib_pixel_weight, absgrad,
                  *camera_inputs(raster_settings, camera_grads, camera_model, camera_model_grads), index_maps=index_maps)


def _apply(features, *inputs, distortion=False, median_depth=False, index_maps=None):
    """features=None: the Function of every release so far, on its own inputs; a tensor: the Function that takes it in front of them
    and returns the feature map behind the other outputs.  distortion=True: the Function that returns the distortion map behind
    depth and alpha, with `features` (a tensor or None) in front of the inputs.  median_depth=True or index_maps: the Function that
    takes all four in front of the inputs."""
    if median_depth or index_maps is not None:
        return _RasterizeGaussiansMedian.apply(features, distortion, median_depth, index_maps, *inputs)
    if distortion:
        return _RasterizeGaussiansDistortion.apply(features, *inputs)
    if features is None:
        return _RasterizeGaussians.apply(*inputs)
    return _RasterizeGaussiansFeatures.apply(features, *inputs)


def camera_inputs(raster_settings, camera_grads, camera_model=None, camera_model_grads=False):
    """What the autograd Functions take behind their own inputs.  camera_grads=True: the three camera tensors of the settings; a
    camera model: the checked CameraModel alone (one input that is no tensor); neither: nothing, so a call without either is the call
    it always was.  Anything but a bool raises TypeError; a bad camera model TypeError or ValueError (_C.camera_model); both together
    NotImplementedError.  A camera model with camera_model_grads (True or the intrinsics tensor, _C.camera_model_grads_arg): four
    inputs, the model, the settings' viewmatrix and campos, and the intrinsics tensor or None."""
    cm = _C.camera_model(camera_model)
    _C.camera_model_excludes(cm, _C.camera_flag(camera_grads))
    cmg = _C.camera_model_grads_arg(camera_model_grads, cm)
    if cmg is not False:
        return (cm, raster_settings.viewmatrix, raster_settings.campos, None if cmg is True else cmg)
    if cm is not None:
        return (cm,)
    if not camera_grads:
        return ()
    return (raster_settings.viewmatrix, raster_settings.projmatrix, raster_settings.campos)


def camera_grad_results(needs, grads, inputs):
    """The three camera gradients of a backward, each shaped like its input, None where the input does not require one."""
    return tuple(g.reshape(t.shape) if n else None for n, g, t in zip(needs, grads, inputs))


def camera_model_grad_results(needs, grads, raster_settings):
    """The gradients of the inputs (viewmatrix, campos, intrinsics) behind a CameraModel from a backward's (dL_dviewmatrix,
    dL_dintrinsics, dL_dcampos), None where the input does not require one."""
    dV, dK, dC = grads
    return (dV.reshape(raster_settings.viewmatrix.shape) if needs[0] else None,
            dC.reshape(raster_settings.campos.shape) if needs[1] else None, dK if needs[2] else None)


def rasterize_gaussians_depth_alpha(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                    raster_settings, depth_alpha, densify_stats=None, antialiasing=False, contrib_stats=None,
                                    contrib_pixel_weight=None, camera_grads=False, absgrad=None, features=None, distortion=False,
                                    median_depth=False, index_maps=None, camera_model=None, camera_model_grads=False):
    """rasterize_gaussians() with the depth and alpha maps -> (color, radii, depth (1,H,W), alpha (1,H,W)[, distortion (1,H,W)]
    [, median_depth (1,H,W)][, feature_map])"""
    _C.aux_mode(depth_alpha)
    distortion = _C.distortion_flag(distortion, depth_alpha)
    median_depth = _C.median_flag(median_depth, depth_alpha)
    if index_maps is not None:
        _C.index_map_tensors(index_maps, raster_settings.image_width, raster_settings.image_height)
    return _apply(features, means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                  cov3Ds_precomp, raster_settings, densify_stats, _C.aa_flag(antialiasing), depth_alpha,
                  contrib_stats, contrib_pixel_weight, absgrad,
                  *camera_inputs(raster_settings, camera_grads, camera_model, camera_model_grads),
                  distortion=distortion, median_depth=median_depth, index_maps=index_maps)


class _RasterizeGaussians(torch.autograd.Function):
    """The reference's Function, plus (depth_alpha = "depth" / "invdepth") two differentiable per-pixel outputs from the same blend pass
    (include/gsr_aux.h): depth D = sum_i v_i alpha_i T_i (v_i = view-space z_i for "depth", 1 / z_i for "invdepth"; no background term)
    and alpha A = 1 - T_final.  Colour and radii are bit-identical with and without the maps.  When neither map's gradient reaches the
    backward, the default backward kernels run (the anti-aliased ones with antialiasing=True).

    Camera gradients (include/gsr_cam.h): with the settings' viewmatrix, projmatrix and campos as three more inputs behind the others,
    the backward returns their gradients too -- the camera-gradient kernels run when at least one of the three requires a gradient,
    the default ones otherwise.  The kernels read the tensors of the settings; the inputs only tie them into the graph.

    Absolute gradients (include/gsr_absgrad.h): absgrad = (abs_mean2D, abs_gradient_accum) is checked before anything runs and only
    the backward writes the tensors; a non-tensor input, so the saved tensors stay as they are and the gradient tuple grows by a None.

    Feature channels (include/gsr_features.h): _RasterizeGaussiansFeatures below takes `features` (P, K) in front of these inputs
    and runs this forward and backward with it; through apply() of this class nothing of them is reached.

    Distortion map (include/gsr_distortion.h): _RasterizeGaussiansDistortion below runs this forward with _distortion=True, which
    returns the map behind depth and alpha and saves its per-pixel state behind the aux buffer; the same holds for it.

    Median depth and index maps (include/gsr_median.h): _RasterizeGaussiansMedian below runs this forward with _median and / or
    _index_maps: one launch after the render writes the caller's index tensors in place and, with _median=True, returns the
    median-depth map behind the distortion map's place and saves its state behind the distortion state; the same holds for it.

    Camera model (include/gsr_camera_model.h): a checked CameraModel as the ONE input behind the others (camera_inputs(); never
    together with the three camera tensors) selects the camera-model kernels of the two per-Gaussian stages; the gradient tuple
    grows by a None.

    Camera gradients under a model (include/gsr_cam_cm.h): FOUR inputs behind the others -- the CameraModel, the settings'
    viewmatrix and campos, and the intrinsics tensor (fx, fy, cx, cy) or None -- make the backward return dL/dviewmatrix, dL/dcampos
    and dL/dintrinsics behind the model's None; the camera variant of the camera-model kernels runs when at least one of the three
    requires a gradient, the plain camera-model kernels otherwise.  The kernels read the settings' tensors and the model's floats."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, densify_stats=None, antialiasing=False, depth_alpha=None, contrib_stats=None,
                contrib_pixel_weight=None, absgrad=None, *camera, _features=None, _distortion=False, _median=False,
                _index_maps=None, _lead=None):
        _C.distortion_flag(_distortion, depth_alpha)   # refused before anything runs
        _C.median_flag(_median, depth_alpha)           # the same
        if _index_maps is not None:   # the same
            _C.index_map_tensors(_index_maps, raster_settings.image_width, raster_settings.image_height,
                                 means3D.device if means3D.is_cuda else None)
        if _features is not None:       # the same
            _C.feature_tensor(_features, int(means3D.size(0)), means3D.device if means3D.is_cuda else None)
        if contrib_stats is not None:   # the same
            _C.contrib_stat_tensors(contrib_stats, int(means3D.size(0)))
        if absgrad is not None:         # the same, the render's device included (a CPU means3D is refused by the forward itself)
            _C.absgrad_tensors(absgrad, int(means3D.size(0)), means3D.device if means3D.is_cuda else None)
        # argument order of _C.rasterize_gaussians: reference __init__.py:64-84
        args = (
            raster_settings.bg,
            means3D,
            colors_precomp,
            opacities,
            scales,
            rotations,
            raster_settings.scale_modifier,
            cov3Ds_precomp,
            raster_settings.viewmatrix,
            raster_settings.projmatrix,
            raster_settings.tanfovx,
            raster_settings.tanfovy,
            raster_settings.image_height,
            raster_settings.image_width,
            sh,
            raster_settings.sh_degree,
            raster_settings.campos,
            raster_settings.prefiltered,
            raster_settings.debug,
        )
        # the screen-space filter (include/gsr_aa.h): a keyword of the binding, so the debug snapshot holds the same tuple
        kw = {"antialiasing": True} if antialiasing else {}
        camera_model = camera[0] if len(camera) in (1, 4) else None   # (include/gsr_camera_model.h): a keyword of the binding too
        if camera_model is not None:
            kw["camera_model"] = camera_model
        if len(camera) == 4 and camera[3] is not None and raster_settings.debug:   # the handle of the intrinsics and the model agree
            _C.camera_model_matches(camera_model, camera[3])
        maps = ()
        if depth_alpha is not None:
            num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer, *maps = \
                _C.rasterize_gaussians_depth_alpha(depth_alpha, *args, **kw)
        elif raster_settings.debug:  # reference __init__.py:87-94
            cpu_args = cpu_deep_copy_tuple(args)
            try:
                num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer = _C.rasterize_gaussians(*args, **kw)
            except Exception as ex:
                torch.save(cpu_args, "snapshot_fw.dump")
                print("\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
                raise ex
        else:
            num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer = _C.rasterize_gaussians(*args, **kw)

        if contrib_stats is not None:
            # the blend-weight statistics of this view (include/gsr_contrib.h), from the state the render just left: once per forward,
            # gradients enabled or not, never in backward
            _C.gaussian_contributions(geomBuffer, binningBuffer, imgBuffer, num_rendered, int(means3D.size(0)),
                                      raster_settings.image_width, raster_settings.image_height, contrib_stats, contrib_pixel_weight,
                                      raster_settings.debug)

        fmap = ()
        if _features is not None:
            # the feature map, from the state the render just left and the weights it blended the colours with
            fmap = (_C.features_forward(geomBuffer, binningBuffer, imgBuffer, num_rendered, int(means3D.size(0)),
                                        raster_settings.image_width, raster_settings.image_height, _features, raster_settings.debug),)

        dmap = dstate = ()
        if _distortion:
            # the distortion map, from the same state and weights and the records' depth values
            d, st = _C.distortion_forward(geomBuffer, binningBuffer, imgBuffer, num_rendered, int(means3D.size(0)),
                                          raster_settings.image_width, raster_settings.image_height, raster_settings.debug)
            dmap, dstate = (d,), (st,)

        mmap = mstate = ()
        if _median or _index_maps is not None:
            # the median-depth map and / or the caller's index maps, from the same state: one launch for both, gradients enabled or not
            md, mst = _C.median_forward(geomBuffer, binningBuffer, imgBuffer, num_rendered, int(means3D.size(0)),
                                        raster_settings.image_width, raster_settings.image_height, _index_maps, _median,
                                        raster_settings.debug)
            if _median:
                mmap, mstate = (md,), (mst,)

        ctx.raster_settings = raster_settings
        ctx.densify_stats = densify_stats
        ctx.features = _features is not None   # then input 0 is `features` and every other input sits one place further back
        ctx.distortion = _distortion           # then input 0 is `features` too, a tensor or None
        ctx.median = _median
        # how many inputs of the applied Function sit in front of this class's own
        ctx.lead = _lead if _lead is not None else (1 if (_features is not None or _distortion) else 0)
        ctx.num_rendered = num_rendered
        ctx.antialiasing = antialiasing
        ctx.depth_alpha = depth_alpha
        ctx.camera = len(camera) == 3
        ctx.camera_model = camera_model
        ctx.camera_cm = len(camera) == 4   # viewmatrix, campos and the intrinsics (or None) behind the model (include/gsr_cam_cm.h)
        ctx.absgrad = absgrad
        # after the reference's ten: the aux state of the maps, the distortion map's and the median depth's per-pixel state, and the
        # opacity input that the anti-aliased backward reads (the records hold opacity * rho), each saved on its path only
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer,
                              binningBuffer, imgBuffer, *(() if _features is None else (_features,)), *maps[2:], *dstate, *mstate,
                              *((opacities,) if antialiasing else ()))
        ctx.mark_non_differentiable(radii)
        # no zero tensor for the (integer) radii output on the way back: autograd would fill P words per step for nothing
        ctx.set_materialize_grads(False)
        return (color, radii, *maps[:2], *dmap, *mmap, *fmap)

    @staticmethod
    def backward(ctx, grad_out_color, _, grad_depth=None, grad_alpha=None):
        return _RasterizeGaussians.backward_with(ctx, grad_out_color, grad_depth, grad_alpha, None)[1]

    @staticmethod
    def backward_with(ctx, grad_out_color, grad_depth, grad_alpha, grad_features_map, grad_distortion=None, grad_median=None):
        """-> (dL/dfeatures or None, the gradient tuple of this class's inputs)"""
        num_rendered = ctx.num_rendered
        raster_settings = ctx.raster_settings
        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, binningBuffer,
         imgBuffer, *extra) = ctx.saved_tensors
        off = ctx.lead
        n_in = 15 + (3 if ctx.camera else 0) + (1 if ctx.camera_model is not None else 0) + (3 if ctx.camera_cm else 0)
        fb = None
        if ctx.features:
            features, extra = extra[0], extra[1:]
            if grad_features_map is not None and ctx.needs_input_grad[0] and not any(ctx.needs_input_grad[1:]):
                # features on a frozen scene: their gradient alone, no colour backward, no gradient slots
                return (_C.features_backward_only(geomBuffer, binningBuffer, imgBuffer, num_rendered, int(means3D.size(0)),
                                                  raster_settings.image_width, raster_settings.image_height, features,
                                                  grad_features_map, raster_settings.debug), (None,) * n_in)
            if grad_features_map is not None:   # (no gradient reached the map: the feature pass is skipped)
                fb = _C.FeatureBackward(features, grad_features_map)
        if grad_out_color is None:  # the image took no part in the loss: the zero gradient autograd would have materialised
            grad_out_color = torch.zeros((3, int(raster_settings.image_height), int(raster_settings.image_width)),
                                         dtype=torch.float32, device=means3D.device)
        if ctx.distortion and grad_distortion is not None:
            # (no gradient reached the map: nothing of it runs, and without dL/dD and dL/dA the default backward kernels do)
            kw_dist = {"distortion": _C.DistortionBackward(extra[1], grad_distortion)}
        else:
            kw_dist = {}
        if ctx.median and grad_median is not None:   # the same for the median depth; its state sits behind the distortion state
            kw_dist["median"] = _C.MedianBackward(extra[2 if ctx.distortion else 1], grad_median)
        kw = {"antialiasing": True, "opacities": extra[-1]} if ctx.antialiasing else {}
        cam_needs = tuple(ctx.needs_input_grad[15 + off:18 + off]) if ctx.camera else ()
        if any(cam_needs):
            kw["camera_grads"] = True
        cm_needs = tuple(ctx.needs_input_grad[16 + off:19 + off]) if ctx.camera_cm else ()
        if any(cm_needs):
            kw["camera_model_grads"] = True
        if fb is not None:
            kw["features"] = fb
        if ctx.absgrad is not None:
            kw["absgrad"] = ctx.absgrad
        if ctx.camera_model is not None:
            kw["camera_model"] = ctx.camera_model

        # argument order of _C.rasterize_gaussians_backward: reference __init__.py:118-138
        args = (
            raster_settings.bg,
            means3D,
            radii,
            colors_precomp,
            scales,
            rotations,
            raster_settings.scale_modifier,
            cov3Ds_precomp,
            raster_settings.viewmatrix,
            raster_settings.projmatrix,
            raster_settings.tanfovx,
            raster_settings.tanfovy,
            grad_out_color,
            sh,
            raster_settings.sh_degree,
            raster_settings.campos,
            geomBuffer,
            num_rendered,
            binningBuffer,
            imgBuffer,
            raster_settings.debug,
        )
        if grad_depth is not None or grad_alpha is not None or kw_dist:
            # (the map's gradient alone still takes the aux kernels: they write the slots' dL/dv word and chain it)
            hw = lambda g: None if g is None else g.reshape(g.shape[-2:])
            grads = _C.rasterize_gaussians_backward_depth_alpha(ctx.depth_alpha, *args[:-1], extra[0], hw(grad_depth), hw(grad_alpha),
                                                                raster_settings.debug, stats=ctx.densify_stats, **kw, **kw_dist)
        elif raster_settings.debug and ctx.depth_alpha is None and not any(cam_needs) and not any(cm_needs):  # reference __init__.py:141-148
            cpu_args = cpu_deep_copy_tuple(args)
            try:
                grads = _C.rasterize_gaussians_backward(*args, stats=ctx.densify_stats, **kw)
            except Exception as ex:
                torch.save(cpu_args, "snapshot_bw.dump")
                print("\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
                raise ex
        else:
            # gradients of inputs that were not provided have no consumer below: the binding skips them.  (Neither map in the loss:
            # the default backward kernels, at the default cost.)
            grads = _C.rasterize_gaussians_backward(*args, lean=not raster_settings.debug, stats=ctx.densify_stats, **kw)
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh, grad_scales,
         grad_rotations) = grads[:8]
        cam_grads = ()
        if ctx.camera:
            cam_grads = camera_grad_results(cam_needs, grads[8:], (raster_settings.viewmatrix, raster_settings.projmatrix,
                                                                   raster_settings.campos)) if any(cam_needs) else (None, None, None)
        if ctx.camera_cm:
            cam_grads = camera_model_grad_results(cm_needs, grads[8:], raster_settings) if any(cm_needs) else (None, None, None)

        # gradient order: reference __init__.py:154-164
        grad_features = None
        if fb is not None:   # (no Gaussian: nothing ran)
            grad_features = fb.grad if fb.grad is not None else torch.zeros_like(fb.features)
        return grad_features, (
            grad_means3D,
            grad_means2D,
            grad_sh if (sh.numel() != 0 and grad_sh is not None) else None,
            grad_colors_precomp if colors_precomp.numel() != 0 else None,
            grad_opacities,
            grad_scales if scales.numel() != 0 else None,
            grad_rotations if rotations.numel() != 0 else None,
            grad_cov3Ds_precomp if cov3Ds_precomp.numel() != 0 else None,
            None,
            None,
            None,
            None,
            None,
            None,
            None,
            *(cam_grads if ctx.camera else ()),
            *((None,) if ctx.camera_model is not None else ()),
            *(cam_grads if ctx.camera_cm else ()),
        )


class _RasterizeGaussiansFeatures(torch.autograd.Function):
    """_RasterizeGaussians with `features` (P, K) in front of its inputs -> (color, radii[, depth, alpha], feature_map (K, H, W)):
    feature_map = sum_i features[i] alpha_i T_i with the colour pass's own weights, differentiable w.r.t. features and, through the
    gradient slots of the colour backward, w.r.t. every geometry input (include/gsr_features.h).  Colour, radii and maps have the
    bits of _RasterizeGaussians."""

    @staticmethod
    def forward(ctx, features, *inputs):
        return _RasterizeGaussians.forward(ctx, *inputs, _features=features)

    @staticmethod
    def backward(ctx, grad_out_color, _, *grads):
        grad_depth, grad_alpha = grads[:2] if len(grads) == 3 else (None, None)
        grad_features, rest = _RasterizeGaussians.backward_with(ctx, grad_out_color, grad_depth, grad_alpha, grads[-1])
        return (grad_features, *rest)


class _RasterizeGaussiansDistortion(torch.autograd.Function):
    """_RasterizeGaussians with a depth_alpha mode and the distortion map -> (color, radii, depth, alpha, distortion (1, H, W)
    [, feature_map]): distortion = sum_{j<i} w_i w_j (v_i - v_j)^2 with the colour pass's own weights and the depth values of the
    depth map, differentiable w.r.t. every geometry input through the gradient slots of the aux backward
    (include/gsr_distortion.h).  `features` (P, K) or None sits in front of the inputs, as in _RasterizeGaussiansFeatures.  The other
    outputs have the bits of _RasterizeGaussians."""

    @staticmethod
    def forward(ctx, features, *inputs):
        return _RasterizeGaussians.forward(ctx, *inputs, _features=features, _distortion=True)

    @staticmethod
    def backward(ctx, grad_out_color, _, grad_depth, grad_alpha, grad_distortion, *grad_fmap):
        grad_features, rest = _RasterizeGaussians.backward_with(ctx, grad_out_color, grad_depth, grad_alpha,
                                                                grad_fmap[0] if grad_fmap else None, grad_distortion)
        return (grad_features, *rest)


class _RasterizeGaussiansMedian(torch.autograd.Function):
    """_RasterizeGaussians with the median-depth map and / or the per-pixel index maps (include/gsr_median.h) ->
    (color, radii[, depth, alpha[, distortion][, median_depth (1, H, W)]][, feature_map]).  In front of the inputs: `features` (P, K)
    or None, the distortion and median_depth flags, and index_maps = None or (median_index, dominant_index, dominant_weight), written
    in place by the forward.  median_depth is v of the last blended Gaussian with T > 0.5, differentiable in v only: its gradient is
    added into the aux backward's slots and chained to means3D along the view z axis.  The other outputs have the bits of
    _RasterizeGaussians."""

    @staticmethod
    def forward(ctx, features, distortion, median_depth, index_maps, *inputs):
        return _RasterizeGaussians.forward(ctx, *inputs, _features=features, _distortion=distortion, _median=median_depth,
                                           _index_maps=index_maps, _lead=4)

    @staticmethod
    def backward(ctx, grad_out_color, _, *grads):
        g = list(grads)
        grad_depth, grad_alpha = (g.pop(0), g.pop(0)) if ctx.depth_alpha is not None else (None, None)
        grad_distortion = g.pop(0) if ctx.distortion else None
        grad_median = g.pop(0) if ctx.median else None
        grad_features, rest = _RasterizeGaussians.backward_with(ctx, grad_out_color, grad_depth, grad_alpha, g[0] if g else None,
                                                                grad_distortion, grad_median)
        return (grad_features, None, None, None, *rest)


CameraModel = _C.CameraModel   # (model, fx, fy, cx, cy): the `camera_model` keyword, see GaussianRasterizer


class GaussianRasterizationSettings(NamedTuple):
    """reference __init__.py:168-180"""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


class GaussianRasterizer(nn.Module):
    """reference __init__.py:182-258.

    densify_stats (extension, optional): (xyz_gradient_accum, denom, max_radii2D) float32 [P] tensors that the
    backward's per-Gaussian kernel updates in place for the Gaussians visible in this view -- the bookkeeping of
    train.py:157-159 / scene/gaussian_model.py:599-602 without separate passes (view_parallel.DensificationStats).

    depth_alpha (extension, optional): "depth" or "invdepth" -- forward() then returns (color, radii, depth, alpha) with the
    depth map D = sum_i v_i alpha_i T_i (v_i = view-space z_i, or 1 / z_i; 0 where nothing blends) and the alpha map
    A = 1 - T_final, both (1, H, W) and differentiable, accumulated in the same blend pass as the colour.  Expected depth is D / A.

    antialiasing (extension, default False): upstream's `antialiasing=True`, the screen-space filter of Mip-Splatting.  The projected
    covariance keeps its 0.3 px^2 dilation, and the opacity is scaled by rho = sqrt(max(2.5e-5, det(Sigma) / det(Sigma + 0.3 I))), so a
    sub-pixel Gaussian keeps the footprint integral of its undilated self; gradients include d rho (include/gsr_aa.h).  Combines with
    depth_alpha.  A bool; anything else raises TypeError.

    contrib_stats (extension, optional): (weight_sum, weight_max, pixel_count) -- float32, float32 and int32 [P] tensors, any of them
    None -- that forward() updates in place right after the render, with or without gradients enabled, from the blend weights
    w = alpha * T of this view: weight_sum += sum over pixels of m w, weight_max = max(itself, max w), pixel_count += pixels blended
    into; Gaussians that blended nowhere keep their values, so a sweep over views accumulates (include/gsr_contrib.h).
    contrib_pixel_weight: the map m, (H, W) or (1, H, W) float32, default 1.  The returned tuple is unchanged, and the backward is too.

    camera_grads (extension, default False): with True the settings' viewmatrix, projmatrix and campos take part in autograd as three
    independent inputs, exactly as the kernels read them: a caller who builds full_proj_transform and camera_center from the pose in
    torch gets the total derivative.  The gradients are those of the function the backward differentiates for the Gaussians (clamped
    t.x / t.y constant inside the EWA Jacobian; culling, radii, tile membership and depth order carry none; tanfovx / tanfovy are
    constants).  When none of the three requires a gradient the default kernels run and nothing is allocated.  A bool; anything else
    raises TypeError.

    absgrad (extension, optional): (abs_mean2D, abs_gradient_accum) -- contiguous float32 tensors [P, 2] and [P] on the render's
    device, either of them None -- the absolute screen-space gradients of AbsGS / gsplat's `absgrad` (include/gsr_absgrad.h).  The
    backward overwrites abs_mean2D[g] with (0.5 W sum_p |dL_p/dmean2D.x|, 0.5 H sum_p |dL_p/dmean2D.y|), the moduli taken per pixel
    before any sum -- the units of means2D.grad, exact zeros for Gaussians that blended nowhere -- and adds their norm into
    abs_gradient_accum for the visible Gaussians (radii > 0), the counterpart of densify_stats' xyz_gradient_accum, which stays signed.
    Under no_grad, or when no backward runs, nothing is touched.  Anything but a 2-tuple raises TypeError; wrong tensors ValueError,
    before anything runs.  With None, the default, the default kernels run and every output has the same bits as without the keyword.

    features (extension, a keyword of forward(); default None): a float32 (P, K) HIP tensor of per-Gaussian feature channels, any
    K >= 1 -- semantic or language features, normals, logits.  forward() then returns one more element, LAST in the tuple:
    (color, radii[, depth, alpha], feature_map), feature_map (K, H, W) = sum_i features[i] alpha_i T_i with the weights the colour
    pass blended with, bit for bit; no background term (add (1 - A) bg_k from the alpha map if wanted), zeros where nothing blends.
    One more walk over the tile lists per four channels instead of a whole rasterizer call per three (include/gsr_features.h).
    The map is differentiable w.r.t. features and w.r.t. every geometry input: means2D.grad and densify_stats see the total
    gradient, colour plus features; absgrad stays the colour's moduli alone; contrib_stats is unaffected.  If the map receives no
    gradient its backward pass is skipped; if `features` is the only input that requires a gradient, only dL/dfeatures is computed
    (no colour backward).  A CPU tensor, a wrong dtype or a wrong shape raise before anything runs.  Out of scope, each raising
    NotImplementedError: view_parallel.rasterize_view_parallel and ViewsInFlight with features, and SH-evaluated features (a
    (P, M, K) coefficient tensor).  With None every call form, saved tensor and output is what it was without the keyword.

    distortion (extension, default False; needs depth_alpha): forward() then returns the depth-distortion map behind depth and
    alpha, (color, radii, depth, alpha, distortion[, feature_map]) -- distortion (1, H, W) = sum_{j<i} w_i w_j (v_i - v_j)^2 with
    w = alpha T the colour pass's own weights and v the depth values of the depth map (z for "depth", 1 / z for "invdepth"): the
    per-ray spread of the blend weights along depth, Mip-NeRF 360's distortion loss in the pairwise squared form of 2DGS (gsplat's
    `distloss`).  No background term, 0 where fewer than two Gaussians blend, invariant under v -> v - c and accumulated centred,
    so a far scene keeps its digits (include/gsr_distortion.h).  Differentiable w.r.t. every geometry input, the depths included:
    means2D.grad and densify_stats see the total gradient; absgrad stays the colour's moduli.  When the map's gradient reaches the
    backward the depth-and-alpha backward kernels run, with or without dL/ddepth and dL/dalpha; when it does not, nothing of this
    runs in the backward.  A bool, anything else raises TypeError; True without depth_alpha raises ValueError.  Out of scope
    (NotImplementedError): view_parallel.rasterize_view_parallel and ViewsInFlight.

    median_depth (extension, default False; needs depth_alpha): forward() then returns the median-depth map behind alpha (behind
    distortion when that is present, in front of feature_map, which stays last): (color, radii, depth, alpha[, distortion],
    median_depth[, feature_map]) -- median_depth (1, H, W) = v of the LAST blended Gaussian in front of which the transmittance is
    above 0.5 (2DGS's `if (T > 0.5) median = this`; the last blended Gaussian where T never falls to 0.5), the depth that TSDF fusion
    takes instead of D / A, which floats between surfaces at silhouettes; 0 where nothing blends (include/gsr_median.h).  It is
    differentiable in v only -- dL/dv_i = the sum of the map's gradient over the pixels whose median is i, chained to means3D along
    the view z axis (and to the camera tensors with camera_grads); nothing goes through alpha or T, as in 2DGS and gsplat, so
    means2D.grad, densify_stats and absgrad do not see it.  When the map's gradient reaches the backward the depth-and-alpha backward
    kernels run, with or without dL/ddepth and dL/dalpha; when it does not, nothing of this runs in the backward.  A bool, anything
    else raises TypeError; True without depth_alpha raises ValueError.  Out of scope (NotImplementedError): the view-parallel paths.

    index_maps (extension, optional; with or without depth_alpha): (median_index, dominant_index, dominant_weight) -- contiguous
    int32, int32 and float32 tensors (H, W) or (1, H, W) on the render's device, any of them None -- that forward() overwrites in
    place right after the render, with or without gradients enabled (a no_grad picking pass works): the Gaussian id of the pixel's
    median, the id of the blended Gaussian with the largest weight alpha T (the first in list order on a tie), both -1 where nothing
    blends, and that weight with the forward's bits (0 there).  The per-pixel answer to the question contrib_stats answers per
    Gaussian: picking, lifting 2-D masks to Gaussians, keyframe bookkeeping.  The returned tuple is unchanged; no gradients.  Together
    with median_depth one launch serves both.  Anything but a 3-tuple raises TypeError, wrong tensors ValueError, before anything
    runs.  Out of scope (NotImplementedError): the view-parallel paths.

    camera_model (extension, default None): a CameraModel(model, fx, fy, cx, cy), or the same five values as a plain tuple -- model
    "pinhole" (intrinsics with an off-centre principal point, as COLMAP, TUM, Replica and ScanNet calibrations have) or "fisheye"
    (equidistant, r = f theta, no distortion coefficients); fx, fy in pixels; cx, cy in pixels with the origin at the corner of the
    first pixel and pixel centres at +0.5 (OpenCV / COLMAP).  The default camera is CameraModel("pinhole", W / (2 tanfovx),
    H / (2 tanfovy), W / 2, H / 2).  With a model, viewmatrix, campos, bg, sh_degree, scale_modifier, image_width, image_height,
    prefiltered and debug of the settings keep their meaning; projmatrix, tanfovx and tanfovy are IGNORED.  The near plane
    (view z <= 0.2), the depth order, the depth values of depth_alpha and the SH direction are unchanged; the pinhole's EWA guard
    band follows the principal point (t.x / t.z clamped to [-(cx / fx + 0.3 W / (2 fx)), (W - cx) / fx + 0.3 W / (2 fx)], the default
    path's +-1.3 tanfov at the default intrinsics), the fisheye has the full 2x3 Jacobian and no band (include/gsr_camera_model.h).
    radii, means2D.grad (same units, so densify_stats and absgrad thresholds carry over) and every optional output keep their
    contracts.  Gradients w.r.t. the pose and the intrinsics: camera_model_grads.  Anything but a CameraModel / 5-tuple raises
    TypeError, an unknown model string or a focal length that is not finite and positive ValueError.  Out of scope
    (NotImplementedError, before anything runs): camera_grads=True (its terms differentiate projmatrix; camera_model_grads is the
    form for a model) and the view-parallel paths.  fused_geometry.depth_normals and normal_consistency_loss still assume the
    centred pinhole of tanfovx / tanfovy.  With None every call is what it was without the keyword, bit for bit.

    camera_model_grads (extension, default False; needs camera_model): True makes the settings' viewmatrix and campos autograd
    inputs behind the model, as camera_grads does for the default camera: pose refinement, tracking and bundle adjustment on
    calibrated and fisheye cameras (include/gsr_cam_cm.h).  A float32 (4,) tensor on the render's device does the same and is, in
    addition, the autograd handle of (fx, fy, cx, cy): it receives dL/dintrinsics (self-calibration).  Its VALUES are not read --
    the kernels take the CameraModel's floats; CameraModel.from_tensor(model, intrinsics) builds the model from the tensor (one
    read-back per step), and with settings.debug the forward compares the two and raises ValueError on a mismatch.  The gradients
    are those of the function the camera-model backward differentiates (straight-through 0.99 clamp; the pinhole's guard-band clamp
    a constant, its limits without a gradient w.r.t. the intrinsics; culling, radii, tile membership and depth order carry none);
    projmatrix has none, a model ignores it.  An input that requires no gradient gets None, and when none of the three does the
    plain camera-model kernels run.  Without a camera_model ValueError; anything but a bool or a tensor TypeError; a wrong dtype,
    shape or device ValueError; the view-parallel paths NotImplementedError.  With False every call is the call it was."""

    def __init__(self, raster_settings, densify_stats=None, depth_alpha=None, antialiasing=False, contrib_stats=None,
                 contrib_pixel_weight=None, camera_grads=False, absgrad=None, distortion=False, median_depth=False, index_maps=None,
                 camera_model=None, camera_model_grads=False):
        super().__init__()
        if depth_alpha is not None:
            _C.aux_mode(depth_alpha)   # ValueError for an unknown mode
        self.distortion = _C.distortion_flag(distortion, depth_alpha)   # TypeError for anything but a bool, ValueError without a mode
        self.median_depth = _C.median_flag(median_depth, depth_alpha)   # the same
        # TypeError for anything but a 3-tuple, ValueError for wrong tensors
        if index_maps is not None:
            _C.index_map_tensors(index_maps, raster_settings.image_width, raster_settings.image_height)
        self.index_maps = index_maps
        self.antialiasing = _C.aa_flag(antialiasing)   # TypeError for anything but a bool
        self.camera_grads = _C.camera_flag(camera_grads)   # the same
        # TypeError for anything but a CameraModel / 5-tuple, ValueError for bad values, NotImplementedError with camera_grads
        self.camera_model = _C.camera_model(camera_model)
        _C.camera_model_excludes(self.camera_model, self.camera_grads)
        # ValueError without a model or for a wrong tensor, TypeError for anything but a bool or a tensor
        self.camera_model_grads = _C.camera_model_grads_arg(camera_model_grads, self.camera_model)
        self.raster_settings = raster_settings
        self.densify_stats = densify_stats
        self.depth_alpha = depth_alpha
        self.contrib_stats = contrib_stats
        self.contrib_pixel_weight = contrib_pixel_weight
        self.absgrad = absgrad

    def markVisible(self, positions):
        # Mark visible points (based on frustum culling for camera) with a boolean
        with torch.no_grad():
            raster_settings = self.raster_settings
            visible = _C.mark_visible(positions, raster_settings.viewmatrix, raster_settings.projmatrix)
        return visible

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, features=None):
        raster_settings = self.raster_settings
        if features is not None:   # refused before anything runs
            _C.feature_tensor(features, int(means3D.size(0)))

        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')

        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')

        if shs is None:
            shs = torch.Tensor([])
        if colors_precomp is None:
            colors_precomp = torch.Tensor([])
        if scales is None:
            scales = torch.Tensor([])
        if rotations is None:
            rotations = torch.Tensor([])
        if cov3D_precomp is None:
            cov3D_precomp = torch.Tensor([])

        if self.depth_alpha is not None:
            return rasterize_gaussians_depth_alpha(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                                   cov3D_precomp, raster_settings, self.depth_alpha, self.densify_stats,
                                                   self.antialiasing, self.contrib_stats, self.contrib_pixel_weight, self.camera_grads,
                                                   self.absgrad, features, self.distortion, self.median_depth, self.index_maps,
                                                   self.camera_model, self.camera_model_grads)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                   cov3D_precomp, raster_settings, self.densify_stats, self.antialiasing, self.contrib_stats,
                                   self.contrib_pixel_weight, self.camera_grads, self.absgrad, features, self.index_maps,
                                   self.camera_model, self.camera_model_grads)
