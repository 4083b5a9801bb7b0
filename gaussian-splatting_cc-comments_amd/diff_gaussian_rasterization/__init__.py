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
    options, intrinsics = _C.render_options(raster_settings, None, densify_stats, antialiasing, contrib_stats, contrib_pixel_weight,
                                            camera_grads, absgrad, False, False, index_maps, camera_model, camera_model_grads)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                     raster_settings, options, features, *camera_positions(options, raster_settings, intrinsics))


def rasterize_gaussians_depth_alpha(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                    raster_settings, depth_alpha, densify_stats=None, antialiasing=False, contrib_stats=None,
                                    contrib_pixel_weight=None, camera_grads=False, absgrad=None, features=None, distortion=False,
                                    median_depth=False, index_maps=None, camera_model=None, camera_model_grads=False):
    """rasterize_gaussians() with the depth and alpha maps -> (color, radii, depth (1,H,W), alpha (1,H,W)[, distortion (1,H,W)]
    [, median_depth (1,H,W)][, feature_map])"""
    options, intrinsics = _C.render_options(raster_settings, depth_alpha, densify_stats, antialiasing, contrib_stats,
                                            contrib_pixel_weight, camera_grads, absgrad, distortion, median_depth, index_maps,
                                            camera_model, camera_model_grads, mode_required=True)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                     raster_settings, options, features, *camera_positions(options, raster_settings, intrinsics))


# ---- what the two autograd Functions share (fused_params._RasterizeLeafGaussians is the other one) --------------------------------
# the inputs of both Functions behind `raster_settings`, every one of them None by default
OPTION_INPUTS = ("options", "features", "viewmatrix", "projmatrix", "campos", "intrinsics")


def camera_positions(options, raster_settings, intrinsics):
    """-> (viewmatrix, projmatrix, campos, intrinsics) for apply(): the settings' tensor (the intrinsics: the tensor given as
    camera_model_grads) where options.camera ties that input into the graph, None everywhere else -- a camera tensor whose gradient
    was not asked for is no input, so it cannot make an output require a gradient.  The kernels read the settings and the model's
    floats; the positions only tie the tensors in."""
    if options.camera is None:
        return (None, None, None, None)
    tied = _C.CAMERA_TARGETS[options.camera]
    return tuple((intrinsics if n == "intrinsics" else getattr(raster_settings, n)) if n in tied else None for n in OPTION_INPUTS[2:])


def after_render(ctx, options, features, raster_settings, P, num_rendered, color, radii, maps, state, opacities):
    """What follows the render in every forward: the contrib statistics, the feature map, the distortion map, the median depth and
    index maps, each from the state the render just left; then everything the backward needs goes on ctx, the names of the outputs
    and of the saved tensors included.  maps: () or (depth, alpha, aux state); state: {name: tensor} of what the Function saves for
    its own backward, with "means3D", "geomBuffer", "binningBuffer" and "imgBuffer" among them (extended here).  -> the output tuple
    (color, radii[, depth, alpha][, distortion][, median_depth][, feature_map])."""
    geom, binning, img = state["geomBuffer"], state["binningBuffer"], state["imgBuffer"]
    W, H, debug = raster_settings.image_width, raster_settings.image_height, raster_settings.debug
    outputs, saved = {"color": color, "radii": radii}, state
    if maps:
        outputs["depth"], outputs["alpha"] = maps[:2]
    if options.contrib_stats is not None:   # once per forward, gradients enabled or not, never in backward (include/gsr_contrib.h)
        _C.gaussian_contributions(geom, binning, img, num_rendered, P, W, H, options.contrib_stats, options.contrib_pixel_weight, debug)
    if features is not None:   # with the weights the colours were blended with (include/gsr_features.h)
        feature_map = _C.features_forward(geom, binning, img, num_rendered, P, W, H, features, debug)
        saved["features"] = features
    if maps:
        saved["aux_state"] = maps[2]
    if options.distortion:   # from the same weights and the records' depth values (include/gsr_distortion.h)
        outputs["distortion"], saved["distortion_state"] = _C.distortion_forward(geom, binning, img, num_rendered, P, W, H, debug)
    if options.median_depth or options.index_maps is not None:   # one launch for both (include/gsr_median.h)
        median, median_state = _C.median_forward(geom, binning, img, num_rendered, P, W, H, options.index_maps, options.median_depth,
                                                 debug)
        if options.median_depth:
            outputs["median_depth"], saved["median_state"] = median, median_state
    if features is not None:   # last in the tuple
        outputs["feature_map"] = feature_map
    if options.antialiasing:   # the filter's backward reads the opacity input: the records hold opacity * rho
        saved["opacities"] = opacities
    ctx.raster_settings, ctx.options, ctx.P, ctx.num_rendered = raster_settings, options, P, num_rendered
    ctx.output_names, ctx.saved_names = tuple(outputs), tuple(saved)
    ctx.save_for_backward(*saved.values())   # each on its path only
    ctx.mark_non_differentiable(radii)
    # no zero tensor for the (integer) radii output on the way back: autograd would fill P words per step for nothing
    ctx.set_materialize_grads(False)
    return tuple(outputs.values())


class BackwardPlan(NamedTuple):
    """What before_backward() decided from the output gradients that arrived."""
    needs: dict          # input name -> it requires a gradient
    saved: dict          # saved name -> tensor
    answer: dict         # the frozen-scene short-cut has run: {"features": dL/dfeatures} is the whole backward; else None
    grad_color: torch.Tensor
    map_grads: tuple     # (dL/ddepth, dL/dalpha) as (H, W) or None
    features: object     # _C.FeatureBackward, DistortionBackward, MedianBackward of the maps that took part in the loss, else None
    distortion: object
    median: object
    aux: bool            # the depth-and-alpha backward kernels are needed
    camera: str          # the camera target that is needed ("cam" / "cm"), None when no tied input requires a gradient


def before_backward(ctx, input_names, grad_outputs):
    """What precedes the kernels in every backward.  A map whose gradient did not arrive runs nothing; with neither dL/ddepth,
    dL/dalpha nor a map that chains through the depth values, the default backward kernels run."""
    st = ctx.raster_settings
    needs = dict(zip(input_names, ctx.needs_input_grad))
    grads = dict(zip(ctx.output_names, grad_outputs))
    saved = dict(zip(ctx.saved_names, ctx.saved_tensors))
    grad_map = grads.get("feature_map")
    if grad_map is not None and needs["features"] and not any(v for n, v in needs.items() if n != "features"):
        # features on a frozen scene: their gradient alone, no colour backward, no gradient slots
        answer = {"features": _C.features_backward_only(saved["geomBuffer"], saved["binningBuffer"], saved["imgBuffer"],
                                                        ctx.num_rendered, ctx.P, st.image_width, st.image_height, saved["features"],
                                                        grad_map, st.debug)}
        return BackwardPlan(needs, saved, answer, None, (None, None), None, None, None, False, None)
    features = None if grad_map is None else _C.FeatureBackward(saved["features"], grad_map)
    grad_color = grads["color"]
    if grad_color is None:  # the image took no part in the loss: the zero gradient autograd would have materialised
        grad_color = torch.zeros((3, int(st.image_height), int(st.image_width)), dtype=torch.float32, device=saved["means3D"].device)
    distortion = median = None
    if grads.get("distortion") is not None:
        distortion = _C.DistortionBackward(saved["distortion_state"], grads["distortion"])
    if grads.get("median_depth") is not None:
        median = _C.MedianBackward(saved["median_state"], grads["median_depth"])
    grad_depth, grad_alpha = grads.get("depth"), grads.get("alpha")
    if grad_depth is not None:
        grad_depth = grad_depth.reshape(grad_depth.shape[-2:])
    if grad_alpha is not None:
        grad_alpha = grad_alpha.reshape(grad_alpha.shape[-2:])
    # (the distortion map's or the median depth's gradient alone still takes the aux kernels: they write the slots' dL/dv word and
    # chain it)
    aux = grad_depth is not None or grad_alpha is not None or distortion is not None or median is not None
    camera = ctx.options.camera
    if camera is not None and not any(needs[n] for n in _C.CAMERA_TARGETS[camera]):
        camera = None
    return BackwardPlan(needs, saved, None, grad_color, (grad_depth, grad_alpha), features, distortion, median, aux, camera)


def after_backward(plan, camera_grads, raster_settings):
    """-> {input name: gradient} of `features` and of the tied camera inputs that require one, each shaped like its input;
    camera_grads: the three results of the camera target in the order of _C.CAMERA_TARGETS[plan.camera]."""
    out = {}
    if plan.features is not None:   # (no Gaussian: nothing ran)
        out["features"] = plan.features.grad if plan.features.grad is not None else torch.zeros_like(plan.features.features)
    if plan.camera is not None:
        for n, g in zip(_C.CAMERA_TARGETS[plan.camera], camera_grads):
            if plan.needs[n]:
                out[n] = g if n == "intrinsics" else g.reshape(getattr(raster_settings, n).shape)
    return out


class _RasterizeGaussians(torch.autograd.Function):
    """The reference's Function: its nine inputs, then OPTION_INPUTS -- the checked _C.RenderOptions (None: the defaults), the
    feature channels (P, K) or None, and the four camera tensors, each None unless options.camera ties it into the graph
    (camera_positions()).  What each option does is written at GaussianRasterizer.

    -> (color, radii[, depth, alpha][, distortion][, median_depth][, feature_map]).  Colour, radii and every map have the same bits
    whatever else is returned.  In the backward a map whose gradient did not arrive runs nothing of its own, and when neither
    dL/ddepth, dL/dalpha, dL/ddistortion nor dL/dmedian_depth arrived the default backward kernels run (before_backward()); the camera
    variant of the per-Gaussian kernels runs when at least one tied camera input requires a gradient.

    A new option is one field of the record, one output name and one saved name in after_render() if it has any, and one input
    position here and in _RasterizeLeafGaussians if it is differentiable; inputs, outputs and saved tensors are only ever reached
    by name."""

    INPUTS = ("means3D", "means2D", "sh", "colors_precomp", "opacities", "scales", "rotations", "cov3Ds_precomp",
              "raster_settings") + OPTION_INPUTS

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, options=None, features=None, viewmatrix=None, projmatrix=None, campos=None, intrinsics=None):
        options = _C.RenderOptions() if options is None else options
        P = int(means3D.size(0))
        # refused before anything runs (a CPU means3D is refused by the forward itself)
        _C.check_render_tensors(options, features, intrinsics, P, means3D.device if means3D.is_cuda else None, raster_settings)
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
        # the screen-space filter (include/gsr_aa.h) and the camera model (include/gsr_camera_model.h): keywords of the binding, so
        # the debug snapshot holds the same tuple
        kw = {"antialiasing": True} if options.antialiasing else {}
        if options.camera_model is not None:
            kw["camera_model"] = options.camera_model
        maps = ()
        if options.depth_alpha is not None:
            num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer, *maps = \
                _C.rasterize_gaussians_depth_alpha(options.depth_alpha, *args, **kw)
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
        # the reference's ten saved tensors
        state = dict(colors_precomp=colors_precomp, means3D=means3D, scales=scales, rotations=rotations, cov3Ds_precomp=cov3Ds_precomp,
                     radii=radii, sh=sh, geomBuffer=geomBuffer, binningBuffer=binningBuffer, imgBuffer=imgBuffer)
        return after_render(ctx, options, features, raster_settings, P, num_rendered, color, radii, maps, state, opacities)

    @staticmethod
    def backward(ctx, *grad_outputs):
        plan = before_backward(ctx, _RasterizeGaussians.INPUTS, grad_outputs)
        if plan.answer is not None:
            return tuple(map(plan.answer.get, _RasterizeGaussians.INPUTS))
        raster_settings, options, s = ctx.raster_settings, ctx.options, plan.saved
        kw = {"antialiasing": True, "opacities": s["opacities"]} if options.antialiasing else {}
        if plan.camera == "cam":
            kw["camera_grads"] = True
        if plan.camera == "cm":
            kw["camera_model_grads"] = True
        if plan.features is not None:
            kw["features"] = plan.features
        if options.absgrad is not None:
            kw["absgrad"] = options.absgrad
        if options.camera_model is not None:
            kw["camera_model"] = options.camera_model

        # argument order of _C.rasterize_gaussians_backward: reference __init__.py:118-138
        args = (
            raster_settings.bg,
            s["means3D"],
            s["radii"],
            s["colors_precomp"],
            s["scales"],
            s["rotations"],
            raster_settings.scale_modifier,
            s["cov3Ds_precomp"],
            raster_settings.viewmatrix,
            raster_settings.projmatrix,
            raster_settings.tanfovx,
            raster_settings.tanfovy,
            plan.grad_color,
            s["sh"],
            raster_settings.sh_degree,
            raster_settings.campos,
            s["geomBuffer"],
            ctx.num_rendered,
            s["binningBuffer"],
            s["imgBuffer"],
            raster_settings.debug,
        )
        if plan.aux:
            if plan.distortion is not None:
                kw["distortion"] = plan.distortion
            if plan.median is not None:
                kw["median"] = plan.median
            grads = _C.rasterize_gaussians_backward_depth_alpha(options.depth_alpha, *args[:-1], s["aux_state"], *plan.map_grads,
                                                                raster_settings.debug, stats=options.densify_stats, **kw)
        elif raster_settings.debug and options.depth_alpha is None and plan.camera is None:  # reference __init__.py:141-148
            cpu_args = cpu_deep_copy_tuple(args)
            try:
                grads = _C.rasterize_gaussians_backward(*args, stats=options.densify_stats, **kw)
            except Exception as ex:
                torch.save(cpu_args, "snapshot_bw.dump")
                print("\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
                raise ex
        else:
            # gradients of inputs that were not provided have no consumer below: the binding skips them.  (Neither map in the loss:
            # the default backward kernels, at the default cost.)
            grads = _C.rasterize_gaussians_backward(*args, lean=not raster_settings.debug, stats=options.densify_stats, **kw)
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh, grad_scales,
         grad_rotations) = grads[:8]

        # reference __init__.py:154-164: no gradient for an input that was not provided
        out = after_backward(plan, grads[8:], raster_settings)
        out.update(means3D=grad_means3D, means2D=grad_means2D, opacities=grad_opacities,
                   sh=grad_sh if (s["sh"].numel() != 0 and grad_sh is not None) else None,
                   colors_precomp=grad_colors_precomp if s["colors_precomp"].numel() != 0 else None,
                   scales=grad_scales if s["scales"].numel() != 0 else None,
                   rotations=grad_rotations if s["rotations"].numel() != 0 else None,
                   cov3Ds_precomp=grad_cov3Ds_precomp if s["cov3Ds_precomp"].numel() != 0 else None)
        return tuple(map(out.get, _RasterizeGaussians.INPUTS))   # everything not named: None


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
        # every keyword is checked here, as each call checks it again: the exceptions are those of _C.render_options()
        options, intrinsics = _C.render_options(raster_settings, depth_alpha, densify_stats, antialiasing, contrib_stats,
                                                contrib_pixel_weight, camera_grads, absgrad, distortion, median_depth, index_maps,
                                                camera_model, camera_model_grads)
        self.raster_settings = raster_settings
        self.densify_stats, self.depth_alpha, self.antialiasing = densify_stats, depth_alpha, antialiasing
        self.contrib_stats, self.contrib_pixel_weight, self.absgrad = contrib_stats, contrib_pixel_weight, absgrad
        self.distortion, self.median_depth, self.index_maps = distortion, median_depth, index_maps
        self.camera_grads, self.camera_model = camera_grads, options.camera_model
        self.camera_model_grads = intrinsics if intrinsics is not None else options.camera == "cm"

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
