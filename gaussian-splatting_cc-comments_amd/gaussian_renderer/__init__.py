"""Caller of the rasterizer hot path with the reference's contract
(gaussian_renderer/__init__.py:18-124): `render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier,
override_color)` -> {"render", "viewspace_points", "visibility_filter", "radii"}.

What the contract fixes, and this module keeps:
  * the rasterizer receives ACTIVATED parameters (`pc.get_*`), the camera's `world_view_transform`,
    `full_proj_transform`, `camera_center`, `tan(FoV / 2)` and `pc.active_sh_degree`;
  * a zero (P,3) tensor travels as `means2D`; its `.grad` after backward is dL/d(screen-space mean),
    which densification reads (train.py:157-159) -- it is returned as "viewspace_points";
  * `pipe.convert_SHs_python` evaluates the SH colours in PyTorch and hands them over as
    `colors_precomp`; `pipe.compute_cov3D_python` does the same for the covariance
    (`pc.get_covariance`); `override_color` replaces the colours altogether;
  * `visibility_filter` = `radii > 0`.
`pc` is anything with the read interface of scene/gaussian_model.py:114-138 -- gsr_model.GaussianParams
or the reference's own GaussianModel.

Extension (not in the reference): `pipe.fused_activations = True` renders straight from the optimiser
leaves (`pc._xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation`) with the activations and
their backward done inside the per-Gaussian kernels (fused_params.py) -- same result dict.
`pipe.antialiasing = True` (where upstream's PipelineParams keeps it) renders with the screen-space filter (GaussianRasterizer).
`filter_3d=` renders with Mip-Splatting's 3D smoothing filter folded into the opacities and scales (fused_filter3d).
`time=` renders a model of 4D Gaussians conditioned on that time stamp (fused_slice4d).
"""
import math

import torch

from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
from gsr_model import eval_sh


def _settings_for(camera, pc, pipe, bg_color, scaling_modifier):
    return GaussianRasterizationSettings(
        image_height=int(camera.image_height), image_width=int(camera.image_width),
        tanfovx=math.tan(0.5 * camera.FoVx), tanfovy=math.tan(0.5 * camera.FoVy),
        bg=bg_color, scale_modifier=scaling_modifier,
        viewmatrix=camera.world_view_transform, projmatrix=camera.full_proj_transform,
        sh_degree=pc.active_sh_degree, campos=camera.camera_center,
        prefiltered=False, debug=pipe.debug)


def _python_sh_colors(camera, pc):
    """SH -> RGB outside the kernel (the reference's convert_SHs_python branch)."""
    feats = pc.get_features                                            # (P, (Dmax+1)^2, 3)
    per_channel = feats.transpose(1, 2).view(-1, 3, (pc.max_sh_degree + 1) ** 2)
    view_dir = pc.get_xyz - camera.camera_center.repeat(feats.shape[0], 1)
    view_dir = view_dir / view_dir.norm(dim=1, keepdim=True)
    return torch.clamp_min(eval_sh(pc.active_sh_degree, per_channel, view_dir) + 0.5, 0.0)


def _result(image, screenspace_points, radii, aux=None, feature_map=None, distortion=None, median_depth=None, user_channels=None):
    """user_channels: None, or the number K of the caller's own feature channels in front of the three normal channels of
    render(normals=True): "features" keeps exactly those K (absent for K = 0), "normal" gets the last three"""
    out = {"render": image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0, "radii": radii}
    if aux is not None:
        out["depth"], out["alpha"] = aux
    if distortion is not None:
        out["distortion"] = distortion
    if median_depth is not None:
        out["median_depth"] = median_depth
    if user_channels is not None:
        feature_map, out["normal"] = (feature_map[:user_channels] if user_channels else None), feature_map[user_channels:]
    if feature_map is not None:
        out["features"] = feature_map
    return out


def _gaussian_normals(camera, pc, leaf, camera_grads):
    """(P, 3) per-Gaussian normals for the feature pass, in view space.  The kernel reads the raw leaves on the leaf path (log-scales
    choose the same axis, the quaternion is normalised inside).  With camera gradients it returns world-space normals and the rotation
    into view space is done here in torch, so that world_view_transform receives that gradient."""
    from fused_geometry import gaussian_normals
    scales, rotations = (pc._scaling, pc._rotation) if leaf else (pc.get_scaling, pc.get_rotation)
    if camera_grads:
        return gaussian_normals(scales, rotations, pc.get_xyz, camera.world_view_transform, "world") @ camera.world_view_transform[:3, :3]
    return gaussian_normals(scales, rotations, pc.get_xyz, camera.world_view_transform, "view")


def _unpack(out, depth_alpha, features, distortion=False, median_depth=False):
    """(color, radii[, depth, alpha[, distortion][, median_depth]][, feature_map]) -> the arguments of _result() behind the
    screen-space points"""
    return (out[1], (out[2:4] if depth_alpha is not None else None), (out[-1] if features is not None else None),
            (out[4] if distortion else None), (out[5 if distortion else 4] if median_depth else None))


def render(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None, densify_stats=None,
           depth_alpha=None, antialiasing=None, contrib_stats=None, contrib_pixel_weight=None, camera_grads=None,
           absgrad=None, features=None, distortion=False, median_depth=False, index_maps=None, normals=False, camera_model=None,
           camera_model_grads=None, filter_3d=None, time=None):
    """Render the scene seen from `viewpoint_camera`.  `bg_color` must live on the GPU.
    densify_stats (extension): see GaussianRasterizer -- the statistics of train.py:157-159 updated by the backward.
    depth_alpha (extension): "depth" or "invdepth" adds "depth" and "alpha" (1, H, W) to the dict -- see GaussianRasterizer.
    antialiasing: the screen-space filter with opacity compensation (see GaussianRasterizer); None = getattr(pipe, "antialiasing",
    False).
    contrib_stats / contrib_pixel_weight (extension): see GaussianRasterizer -- the per-Gaussian blend-weight statistics of this view
    (weight sum, weight max, hit count), updated by the forward on both paths.
    camera_grads: the camera's world_view_transform, full_proj_transform and camera_center take part in autograd (see
    GaussianRasterizer): pose refinement; None = getattr(pipe, "camera_grads", False).
    absgrad (extension): (abs_mean2D, abs_gradient_accum), see GaussianRasterizer -- the absolute screen-space gradients, written by the
    backward on both paths; None = off.
    features (extension): a float32 (P, K) tensor of per-Gaussian feature channels adds "features" (K, H, W) to the dict, blended
    with the colour pass's own weights and differentiable -- see GaussianRasterizer; on both paths.
    distortion (extension): True (with depth_alpha) adds "distortion" (1, H, W) to the dict, the depth-distortion map
    sum_{j<i} w_i w_j (v_i - v_j)^2 of the same weights and the depth map's values, differentiable -- see GaussianRasterizer; on
    both paths.
    median_depth (extension): True (with depth_alpha) adds "median_depth" (1, H, W) to the dict, the depth value of the last blended
    Gaussian with T > 0.5, differentiable in that value -- see GaussianRasterizer; on both paths.
    index_maps (extension): (median_index, dominant_index, dominant_weight) tensors that the render overwrites in place -- see
    GaussianRasterizer; the dict is unchanged; on both paths.
    normals (extension): True adds "normal" (3, H, W) to the dict, the blend sum_i n_i alpha_i T_i of the per-Gaussian view-space
    normals of fused_geometry.gaussian_normals(), differentiable (rotations through n_i, everything else through the weights): three
    more channels of the feature pass behind the caller's `features`, split off again -- "features" keeps exactly the caller's
    channels; on both paths.  The input of fused_geometry.normal_consistency_loss().
    camera_model (extension): a CameraModel ("pinhole" with intrinsics, or "fisheye") -- see GaussianRasterizer; None = the camera's own
    `camera_model` attribute if it has one, else the centred pinhole of FoVx / FoVy.  With a model the camera's full_proj_transform,
    FoVx and FoVy are ignored; on both paths; not with camera_grads (camera_model_grads is its form for a model).  The normal map of normals=True is the blend of per-Gaussian
    normals and works with either model; fused_geometry.depth_normals() and normal_consistency_loss(), which the caller applies to the
    result, still assume the centred pinhole.
    camera_model_grads (extension): True, or the float32 (4,) tensor (fx, fy, cx, cy) that is the autograd handle of the model's
    intrinsics -- the camera's world_view_transform and camera_center (and the tensor) take part in autograd behind the camera
    model (see GaussianRasterizer): pose refinement and self-calibration on calibrated and fisheye cameras; None =
    getattr(pipe, "camera_model_grads", False); on both paths.
    filter_3d (extension): the float32 (P, 1) tensor of fused_filter3d.compute_filter_3d() -- Mip-Splatting's 3D smoothing filter: the
    rasterizer receives fused_filter3d.filtered_activations(pc._opacity, pc._scaling, filter_3d) as its opacities and scales, and the
    gradients reach the two leaves through that function's backward.  Always the GaussianRasterizer path, under
    pipe.fused_activations too: the two per-Gaussian leaf kernels do not know the filter, and teaching them means new instantiations
    across every variant of both (a follow-up).  Not with pipe.compute_cov3D_python (NotImplementedError): the covariance of
    pc.get_covariance() carries no filter.
    time (extension): a Python float -- `pc` is a model of 4D Gaussians (Yang et al., "Real-time Photorealistic Dynamic Scene
    Representation and Rendering with 4D Gaussian Splatting") and must carry `_t` (P,1), `_scaling_t` (P,1) and `_rotation_r` (P,4) beside
    the usual leaves (TypeError otherwise, before anything runs).  The rasterizer receives fused_slice4d.slice_at(pc._xyz, pc._t,
    pc._scaling, pc._scaling_t, pc._rotation, pc._rotation_r, pc._opacity, time, scaling_modifier) as its means3D, cov3D_precomp and
    opacities, and the gradients reach the seven leaves through that function's backward.  If `pc` has `_features_t` (P, N+1, M, 3)
    (with `pc.time_period`) the rasterizer receives fused_slice4d.harmonic_features(pc._features_t, pc._t, time, pc.time_period) as its
    shs, otherwise pc.get_features.  Always the GaussianRasterizer path, as with filter_3d; every other extension keyword works
    unchanged on top.  "viewspace_points" is zeros_like of the sliced means; "visibility_filter" is (radii > 0) &
    fused_slice4d.visible_at(opacities): a Gaussian whose temporal marginal is at or below the cutoff is not visible.  "radii" and the
    denominators of densify_stats are not touched: a masked Gaussian inside the frustum still has its radius and still counts there.
    Not with filter_3d, pipe.compute_cov3D_python or pipe.convert_SHs_python (NotImplementedError).  None: today's code path."""
    from diff_gaussian_rasterization import _C
    _C.normals_flag(normals)   # a switch: anything but a bool is refused
    if camera_model is None:
        camera_model = getattr(viewpoint_camera, "camera_model", None)
    if camera_grads is None:
        camera_grads = getattr(pipe, "camera_grads", False)
    camera_model = _C.camera_model(camera_model)   # refused before anything runs: a bad model, and a model with camera gradients
    _C.camera_model_excludes(camera_model, camera_grads is True)
    if camera_model_grads is None:
        camera_model_grads = getattr(pipe, "camera_model_grads", False)
    camera_model_grads = _C.camera_model_grads_arg(camera_model_grads, camera_model)   # refused before anything runs too
    if antialiasing is None:
        antialiasing = getattr(pipe, "antialiasing", False)
    if time is not None:   # refused before anything runs too
        import fused_slice4d
        missing = [n for n in ("_t", "_scaling_t", "_rotation_r") if not hasattr(pc, n)]
        if missing:
            raise TypeError(f"time=: the model must carry _t, _scaling_t and _rotation_r (4D Gaussians); it lacks {', '.join(missing)}")
        for on, what in ((filter_3d is not None, "filter_3d"), (bool(pipe.compute_cov3D_python), "pipe.compute_cov3D_python"),
                         (bool(pipe.convert_SHs_python), "pipe.convert_SHs_python")):
            if on:
                raise NotImplementedError(f"time= with {what}: the time slice hands the rasterizer its own covariance, opacities and SH coefficients")
        leaves4d = (pc._xyz, pc._t, pc._scaling, pc._scaling_t, pc._rotation, pc._rotation_r, pc._opacity)
        fused_slice4d._check(**dict(zip(fused_slice4d.LEAVES, leaves4d)))
        fused_slice4d._check_scalars(time, scaling_modifier, 0.05)
        harmonics = hasattr(pc, "_features_t")
        if harmonics:
            fused_slice4d._check(t=pc._t, features_t=pc._features_t)
            fused_slice4d._check_period(pc.time_period)
        fused_slice4d._check_device(*leaves4d, *((pc._features_t,) if harmonics else ()))
        sliced = fused_slice4d.slice_at(*leaves4d, float(time), scaling_modifier=float(scaling_modifier))
    if filter_3d is not None:   # refused before anything runs, and before the kernel library is loaded
        import fused_filter3d
        if bool(pipe.compute_cov3D_python):
            raise NotImplementedError("filter_3d with pipe.compute_cov3D_python: pc.get_covariance() carries no 3D filter")
        fused_filter3d._check(opacity=pc._opacity, scaling=pc._scaling, filter_3d=filter_3d)
        fused_filter3d._check_device(pc._opacity, pc._scaling, filter_3d)
    xyz = pc.get_xyz if time is None else sliced[0]
    # carrier of the screen-space gradient: zeros, a non-leaf that keeps its grad
    screenspace_points = torch.zeros_like(xyz, dtype=xyz.dtype, requires_grad=True, device=xyz.device) + 0
    try:
        screenspace_points.retain_grad()
    except Exception:
        pass
    settings = _settings_for(viewpoint_camera, pc, pipe, bg_color, scaling_modifier)
    # the optional extensions travel only when asked for, as more keywords of either path: the blend-weight statistics ...
    extras = {} if contrib_stats is None else dict(contrib_stats=contrib_stats, contrib_pixel_weight=contrib_pixel_weight)
    if camera_grads is not False:   # the camera gradients travel the same way (a non-bool reaches the check that refuses it)
        extras["camera_grads"] = camera_grads
    if absgrad is not None:
        extras["absgrad"] = absgrad
    python_cov = bool(pipe.compute_cov3D_python)
    python_sh = bool(pipe.convert_SHs_python)
    leaf = bool(getattr(pipe, "fused_activations", False)) and override_color is None and not python_cov and not python_sh and filter_3d is None and time is None
    user_channels = None
    if normals:   # three more feature channels behind the caller's own
        n = _gaussian_normals(viewpoint_camera, pc, leaf, camera_grads is True or camera_model_grads is not False)
        if features is None:
            user_channels, features = 0, n
        else:
            user_channels = _C.feature_tensor(features, xyz.size(0), xyz.device)
            features = torch.cat((features, n), dim=1)
    feat = {} if features is None else dict(features=features)   # ... and the feature channels, a keyword of the call itself
    if distortion is not False:   # ... and the distortion map (a non-bool reaches the check that refuses it)
        extras["distortion"] = distortion
    if median_depth is not False:   # ... the median-depth map, the same way
        extras["median_depth"] = median_depth
    if index_maps is not None:      # ... and the caller's index maps
        extras["index_maps"] = index_maps
    if camera_model is not None:    # ... and the camera model (checked by either path before anything runs)
        extras["camera_model"] = camera_model
    if camera_model_grads is not False:   # ... with the camera gradients under it
        extras["camera_model_grads"] = camera_model_grads

    if leaf:
        from fused_params import rasterize_leaf_gaussians
        out = rasterize_leaf_gaussians(pc._xyz, screenspace_points, pc._features_dc, pc._features_rest, pc._opacity,
                                       pc._scaling, pc._rotation, settings, densify_stats, depth_alpha=depth_alpha,
                                       antialiasing=antialiasing, **feat, **extras)
        return _result(out[0], screenspace_points, *_unpack(out, depth_alpha, features, distortion, median_depth),
                       user_channels=user_channels)

    inputs = dict(means3D=xyz, means2D=screenspace_points, opacities=pc.get_opacity if time is None else sliced[2],
                  shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None)
    if time is not None:
        inputs["cov3D_precomp"] = sliced[1]
    elif python_cov:
        inputs["cov3D_precomp"] = pc.get_covariance(scaling_modifier)
    else:
        inputs["scales"], inputs["rotations"] = pc.get_scaling, pc.get_rotation
    if filter_3d is not None:
        inputs["opacities"], inputs["scales"] = fused_filter3d.filtered_activations(pc._opacity, pc._scaling, filter_3d)
    if override_color is not None:
        inputs["colors_precomp"] = override_color
    elif python_sh:
        inputs["colors_precomp"] = _python_sh_colors(viewpoint_camera, pc)
    elif time is not None and harmonics:
        inputs["shs"] = fused_slice4d.harmonic_features(pc._features_t, pc._t, float(time), float(pc.time_period))
    else:
        inputs["shs"] = pc.get_features

    out = GaussianRasterizer(raster_settings=settings, densify_stats=densify_stats, depth_alpha=depth_alpha,
                             antialiasing=antialiasing, **extras)(**inputs, **feat)
    result = _result(out[0], screenspace_points, *_unpack(out, depth_alpha, features, distortion, median_depth),
                     user_channels=user_channels)
    if time is not None:
        result["visibility_filter"] = result["visibility_filter"] & fused_slice4d.visible_at(sliced[2])
    return result
