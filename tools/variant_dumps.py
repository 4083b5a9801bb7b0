"""One seeded forward + backward of every variant of the Python binding, dumped as .npy for a byte-for-byte comparison of two trees
(tools/compare_dumps.py): the same library behind two versions of the Python drivers must give the same bytes.

    python tools/variant_dumps.py TREE OUT_DIR [--points 4000]

TREE is the checkout to import from (its own built libgsr_hip.so); only names that every version of the package has are used:
GaussianRasterizer, fused_params.rasterize_leaf_gaussians, view_parallel.rasterize_view_parallel (one rank).  Variants:
{plain, leaf} x {no maps, "depth", "invdepth"} x {filter off, on}; the plain path with precomputed colours and covariances; the plain
path with densification statistics; the view-parallel path with the filter off and on.  The loss uses every output (random upstream
gradients for image, depth and alpha).  Written per variant: every output, every input gradient, the statistics tensors.

The options, each through GaussianRasterizer ("plain_opt_*") and rasterize_leaf_gaussians ("leaf_opt_*"): features (K = 1 and 5);
distortion, median_depth and index_maps alone and all together with features; camera_grads; camera_model pinhole and fisheye;
camera_model_grads as True and as the intrinsics tensor; absgrad; contrib_stats with a pixel weight; the frozen scene where only
`features` requires a gradient; and one case per map where the map is produced and takes no part in the loss.  Written per case:
every output, the gradient of every input (the camera tensors and the intrinsics count as inputs; an input without a gradient is
written as an empty array) and every tensor written in place (index maps, absgrad, contrib and densification statistics).
"""
import argparse
import os
import sys

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("tree")
    ap.add_argument("out_dir")
    ap.add_argument("--points", type=int, default=4000)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    for p in (tree, os.path.join(tree, "gaussian-splatting_cc-comments_amd")):
        sys.path.insert(0, p)
    import fused_params
    import gsr_model
    import gsr_scene
    import view_parallel
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C
    assert os.path.abspath(_C.__file__).startswith(tree + os.sep), _C.__file__

    dev = torch.device("cuda:0")
    P, D = args.points, 3
    scene = gsr_scene.make_scene(P, -3.0, sh_degree=D, seed=11)
    cam = gsr_scene.make_camera(320, 200)
    H, W = cam.image_height, cam.image_width
    st = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=scene.bg.to(dev), scale_modifier=1.0,
        viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev), sh_degree=D,
        campos=cam.camera_center.to(dev), prefiltered=False, debug=False)
    g = torch.Generator().manual_seed(5)
    ups = [torch.randn(c, H, W, generator=g).to(dev) for c in (3, 1, 1)]   # dL/dimage, dL/ddepth, dL/dalpha
    os.makedirs(args.out_dir, exist_ok=True)

    def finish(tag, outs, inputs, stats=None):
        color, radii, *maps = outs
        loss = sum((o * u).sum() for o, u in zip([color] + maps, ups))
        loss.backward()
        torch.cuda.synchronize()
        arrays = {"color": color, "radii": radii}
        arrays.update({n: m for n, m in zip(("depth", "alpha"), maps)})
        arrays.update({"grad_" + n: t.grad for n, t in inputs.items()})
        arrays.update({"stat_" + n: t for n, t in zip(("xyz_gradient_accum", "denom", "max_radii2D"), stats or ())})
        for n, t in arrays.items():
            assert t is not None, (tag, n)
            np.save(os.path.join(args.out_dir, f"{tag}.{n}.npy"), t.detach().cpu().numpy())
        print(f"{tag}: {len(arrays)} arrays", flush=True)

    def activated():
        t = {k: getattr(scene, k).to(dev).clone().requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
        t["means2D"] = torch.zeros_like(t["means3D"], requires_grad=True)
        return t

    def new_stats():
        return tuple(torch.zeros(P, device=dev) for _ in range(3))

    for mode in (None, "depth", "invdepth"):
        for aa in (False, True):
            tag = f"{mode or 'nomaps'}_{'aa' if aa else 'noaa'}"
            t = activated()
            finish("plain_" + tag, GaussianRasterizer(st, depth_alpha=mode, antialiasing=aa)(**t), t)
            pc = gsr_model.GaussianParams.from_activated(scene.means3D, scene.shs, scene.scales, scene.rotations, scene.opacities,
                                                         device=dev)
            means2D = torch.zeros_like(pc._xyz, requires_grad=True)
            stats = new_stats()
            outs = fused_params.rasterize_leaf_gaussians(pc._xyz, means2D, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling,
                                                         pc._rotation, st, stats=stats, depth_alpha=mode, antialiasing=aa)
            finish("leaf_" + tag, outs, dict(zip(("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity"),
                                                 pc.parameters()), means2D=means2D), stats)

    for aa in (False, True):   # precomputed colours and covariances, with the maps (their backward is the lean set with both present)
        for mode in (None, "depth"):
            t = activated()
            t["colors_precomp"] = torch.rand(P, 3, generator=g).to(dev).requires_grad_(True)
            t["cov3D_precomp"] = gsr_model.build_covariance_from_scaling_rotation(scene.scales, 1.0, scene.rotations).to(dev) \
                .requires_grad_(True)
            for k in ("shs", "scales", "rotations"):
                del t[k]
            finish(f"precomp_{mode or 'nomaps'}_{'aa' if aa else 'noaa'}",
                   GaussianRasterizer(st, depth_alpha=mode, antialiasing=aa)(**t), t)

    for mode, aa in ((None, False), (None, True), ("depth", False), ("depth", True)):   # densification statistics on
        t, stats = activated(), new_stats()
        finish(f"stats_{mode or 'nomaps'}_{'aa' if aa else 'noaa'}",
               GaussianRasterizer(st, densify_stats=stats, depth_alpha=mode, antialiasing=aa)(**t), t, stats)

    for sh_mode in ("compact", "allreduce"):
        for aa in (False, True):
            t, stats = activated(), new_stats()
            ex = view_parallel.GradientExchange(P, scene.shs.shape[1], dev, sh_mode=sh_mode, parts=3)
            outs = view_parallel.rasterize_view_parallel(t["means3D"], t["means2D"], t["shs"], t["opacities"], t["scales"],
                                                         t["rotations"], st, ex, stats=stats, antialiasing=aa)
            finish(f"viewparallel_{sh_mode}_{'aa' if aa else 'noaa'}", outs, t, stats)

    # ---- the options -----------------------------------------------------------------------------------------------------------------
    fx, fy = W / (2.0 * cam.tanfovx), H / (2.0 * cam.tanfovy)
    pinhole, fisheye = ("pinhole", 0.9 * fx, 0.95 * fy, 0.5 * W + 7.3, 0.5 * H - 4.6), ("fisheye", 0.8 * fx, 0.8 * fx, 0.5 * W, 0.5 * H)
    up = {"color": ups[0], "depth": ups[1], "alpha": ups[2], "distortion": torch.randn(1, H, W, generator=g).to(dev),
          "median_depth": torch.randn(1, H, W, generator=g).to(dev), "feature_map": torch.randn(5, H, W, generator=g).to(dev)}
    feats = torch.randn(P, 5, generator=g)
    pixel_weight = torch.rand(H, W, generator=g).to(dev)

    def option_case(kind, tag, opts, K=0, loss=None, camera=None, frozen=False, intrinsics=False):
        """opts: keywords of both entry points but for placeholders: index_maps / absgrad / contrib_stats / stats = True make fresh
        tensors.  loss: the outputs in the loss (default: all).  camera: which tensors of the settings require a gradient."""
        opts, inplace, inputs, s = dict(opts), {}, {}, st
        fresh = {"index_maps": lambda: (torch.zeros(H, W, dtype=torch.int32, device=dev), torch.zeros(1, H, W, dtype=torch.int32, device=dev),
                                        torch.zeros(H, W, device=dev)),
                 "absgrad": lambda: (torch.zeros(P, 2, device=dev), torch.zeros(P, device=dev)),
                 "contrib_stats": lambda: (torch.zeros(P, device=dev), torch.zeros(P, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)),
                 "stats": new_stats}
        for k, make in fresh.items():
            if opts.get(k) is True:
                opts[k] = make()
                inplace.update({f"{k}{i}": t for i, t in enumerate(opts[k])})
        if camera:
            tensors = {n: getattr(st, n).clone().requires_grad_(True) for n in camera}
            s = st._replace(**tensors)
            inputs.update(tensors)
        if intrinsics:
            opts["camera_model_grads"] = inputs["intrinsics"] = torch.tensor(opts["camera_model"][1:], device=dev, requires_grad=True)
        f = feats[:, :K].contiguous().to(dev).requires_grad_(True) if K else None
        if kind == "plain":
            t = activated()
            if "stats" in opts:
                opts["densify_stats"] = opts.pop("stats")
            outs = GaussianRasterizer(s, **opts)(**{k: v.requires_grad_(not frozen) for k, v in t.items()}, features=f)
        else:
            pc = gsr_model.GaussianParams.from_activated(scene.means3D, scene.shs, scene.scales, scene.rotations, scene.opacities,
                                                         device=dev, requires_grad=not frozen)
            t = dict(zip(("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity"), pc.parameters()),
                     means2D=torch.zeros_like(pc._xyz, requires_grad=not frozen))
            outs = fused_params.rasterize_leaf_gaussians(pc._xyz, t["means2D"], pc._features_dc, pc._features_rest, pc._opacity,
                                                         pc._scaling, pc._rotation, s, features=f, **opts)
        inputs.update(t)
        if f is not None:
            inputs["features"] = f
        names = ["color", "radii"] + (["depth", "alpha"] if opts.get("depth_alpha") else []) + \
            [n for n in ("distortion", "median_depth") if opts.get(n)] + (["feature_map"] if K else [])
        assert len(outs) == len(names), (tag, len(outs), names)
        res = dict(zip(names, outs))
        sum((res[n] * up[n][:res[n].shape[0]]).sum() for n in (loss or names) if n != "radii").backward()
        torch.cuda.synchronize()
        arrays = dict(res)
        arrays.update({"grad_" + n: (torch.empty(0) if v.grad is None else v.grad) for n, v in inputs.items()})
        arrays.update({"inplace_" + n: v for n, v in inplace.items()})
        for n, v in arrays.items():
            np.save(os.path.join(args.out_dir, f"{kind}_opt_{tag}.{n}.npy"), v.detach().cpu().numpy())
        print(f"{kind}_opt_{tag}: {len(arrays)} arrays", flush=True)

    everything = dict(depth_alpha="invdepth", distortion=True, median_depth=True)
    for kind in ("plain", "leaf"):
        option_case(kind, "features_k1", {}, K=1)
        option_case(kind, "features_k5", dict(depth_alpha="depth"), K=5)
        option_case(kind, "distortion", dict(depth_alpha="depth", distortion=True))
        option_case(kind, "median_depth", dict(depth_alpha="depth", median_depth=True))
        option_case(kind, "index_maps", dict(index_maps=True))
        option_case(kind, "all_maps_features", dict(everything, index_maps=True, antialiasing=True, stats=True), K=5)
        option_case(kind, "camera_grads", dict(camera_grads=True, depth_alpha="depth"), camera=("viewmatrix", "projmatrix", "campos"))
        option_case(kind, "camera_model_pinhole", dict(camera_model=pinhole))
        option_case(kind, "camera_model_fisheye", dict(camera_model=fisheye, depth_alpha="depth"))
        option_case(kind, "camera_model_grads_true", dict(camera_model=pinhole, camera_model_grads=True), camera=("viewmatrix", "campos"))
        option_case(kind, "camera_model_grads_tensor", dict(camera_model=fisheye, depth_alpha="depth"), camera=("viewmatrix", "campos"),
                    intrinsics=True)
        option_case(kind, "absgrad", dict(absgrad=True, stats=True))
        option_case(kind, "contrib_stats", dict(contrib_stats=True, contrib_pixel_weight=pixel_weight))
        option_case(kind, "frozen_features", dict(depth_alpha="depth"), K=5, frozen=True)
        for unused in (("depth", "alpha"), ("distortion",), ("median_depth",), ("feature_map",)):
            used = [n for n in ("color", "depth", "alpha", "distortion", "median_depth", "feature_map") if n not in unused]
            option_case(kind, "unused_" + unused[0], everything, K=5, loss=used)


if __name__ == "__main__":
    main()
