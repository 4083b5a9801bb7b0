"""Every output of the tile-list replay passes (csrc/gsr_replay.h: contrib.hip, features.hip, distortion.hip, median.hip), dumped as
.npy for a byte-for-byte comparison of two builds of the library (tools/compare_dumps.py), in the manner of tools/variant_dumps.py.

    python tools/replay_dumps.py LIBRARY OUT_DIR

LIBRARY is bound through _C.use_library in this (fresh) process.  Scenes: A = make_scene(2000, -3.0, sh_degree=1, seed=33) at
33 x 17 (a one-pixel tile row and column, one list of at least 1 024), B = make_scene(3000, -3.0, sh_degree=1, seed=21) at 120 x 90;
each with the culling on and with GSR_DEBUG_NO_CULL.  Written per scene and switch:
  direct calls on the state of a depth-and-alpha forward: the contribution statistics without and with a pixel weight; the feature
  forward and the features-only backward (into_slots = 0) at K = 1, 4, 7; the distortion forward (map and state); the median
  forward with all outputs from both instantiations (early exit, GSR_DEBUG_MEDIAN_FULL_WALK);
  one GaussianRasterizer call per K = 1, 4, 7 with features, distortion, median depth and index maps in the loss: every output and
  every input gradient -- the feature backward into the gradient slots, the distortion and median backward, and the per-Gaussian
  backward after their additions.
"""
import argparse
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "gaussian-splatting_cc-comments_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch  # noqa: E402

import gsr_scene  # noqa: E402
from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C  # noqa: E402

SCENES = {"A": (2000, 33, 33, 17), "B": (3000, 21, 120, 90)}   # P, seed, W, H
D, MODE = 1, "depth"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("library")
    ap.add_argument("out_dir")
    args = ap.parse_args()
    _C.use_library(args.library)
    dev = torch.device("cuda:0")
    os.makedirs(args.out_dir, exist_ok=True)
    count = 0

    def save(tag, **arrays):
        nonlocal count
        for n, t in arrays.items():
            assert t is not None, (tag, n)
            np.save(os.path.join(args.out_dir, f"{tag}.{n}.npy"), t.detach().cpu().numpy())
            count += 1

    for name, (P, seed, W, H) in SCENES.items():
        scene, cam = gsr_scene.make_scene(P, -3.0, sh_degree=D, seed=seed), gsr_scene.make_camera(W, H)
        to = lambda t: t.to(dev).contiguous()
        e = torch.empty(0, device=dev)
        gen = torch.Generator().manual_seed(7)
        weight = to(torch.rand(H, W, generator=gen) * 1.5 + 0.25)
        feats = {K: torch.randn(P, K, generator=gen) for K in (1, 4, 7)}
        dmap = {K: to(torch.randn(K, H, W, generator=gen)) for K in (1, 4, 7)}
        dpix = to(torch.randn(3, H, W, generator=gen))
        g1 = [to(torch.randn(1, H, W, generator=gen)) for _ in range(4)]   # dL/ddepth, dL/dalpha, dL/ddistortion, dL/dmedian
        for label, debug in (("cull", 0), ("nocull", _C.DEBUG_NO_CULL)):
            tag = f"{name}_{label}"
            st = GaussianRasterizationSettings(
                image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=to(scene.bg), scale_modifier=1.0,
                viewmatrix=to(cam.world_view_transform), projmatrix=to(cam.full_proj_transform), sh_degree=D, campos=to(cam.camera_center),
                prefiltered=False, debug=debug)
            r = _C.rasterize_gaussians_depth_alpha(MODE, st.bg, to(scene.means3D), e, to(scene.opacities), to(scene.scales), to(scene.rotations),
                                                   1.0, e, st.viewmatrix, st.projmatrix, st.tanfovx, st.tanfovy, H, W, to(scene.shs), D, st.campos,
                                                   False, debug)
            num, color, radii, geom, binning, img = r[:6]
            if name == "A" and label == "cull":
                il = _C.image_layout(W, H)
                T = ((W + 15) // 16) * ((H + 15) // 16)
                rng = img[il.ranges:il.ranges + 8 * T].view(torch.int32).view(T, 2)
                assert int((rng[:, 1] - rng[:, 0]).max()) >= 1024, "scene A no longer has a heavy tile"
            save(tag, color=color, radii=radii)
            for wl, m in (("m1", None), ("map", weight)):
                s = (torch.zeros(P, device=dev), torch.zeros(P, device=dev), torch.zeros(P, dtype=torch.int32, device=dev))
                _C.gaussian_contributions(geom, binning, img, num, P, W, H, s, m, debug)
                save(f"{tag}.contrib_{wl}", weight_sum=s[0], weight_max=s[1], pixel_count=s[2])
            for K in (1, 4, 7):
                f = to(feats[K])
                save(f"{tag}.features_K{K}", forward=_C.features_forward(geom, binning, img, num, P, W, H, f, debug),
                     backward_only=_C.features_backward_only(geom, binning, img, num, P, W, H, f, dmap[K], debug))
            dist, dstate = _C.distortion_forward(geom, binning, img, num, P, W, H, debug)
            save(f"{tag}.distortion", map=dist, state=dstate)
            for tw, md in (("exit", debug), ("fullwalk", debug | _C.DEBUG_MEDIAN_FULL_WALK)):
                im = (torch.full((H, W), -7, dtype=torch.int32, device=dev), torch.full((H, W), -7, dtype=torch.int32, device=dev),
                      torch.full((H, W), -7.0, device=dev))
                med, mstate = _C.median_forward(geom, binning, img, num, P, W, H, index_maps=im, debug=md)
                save(f"{tag}.median_{tw}", depth=med, state=mstate, median_index=im[0], dominant_index=im[1], dominant_weight=im[2])
            # the module: all four passes in one backward, into the gradient slots, then the per-Gaussian backward
            for K in (1, 4, 7):
                t = {k: to(getattr(scene, k)).clone().requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
                t["means2D"] = torch.zeros(P, 3, device=dev, requires_grad=True)
                f = to(feats[K]).clone().requires_grad_(True)
                out = GaussianRasterizer(st, depth_alpha=MODE, distortion=True, median_depth=True)(**t, features=f)
                color, radii, depth, alpha, dist, med, fmap = out
                loss = (color * dpix).sum() + (depth * g1[0]).sum() + (alpha * g1[1]).sum() + (dist * g1[2]).sum() + (med * g1[3]).sum() + \
                    (fmap * dmap[K]).sum()
                loss.backward()
                torch.cuda.synchronize()
                save(f"{tag}.module_K{K}", color=color, depth=depth, alpha=alpha, distortion=dist, median=med, features=fmap,
                     grad_features=f.grad, **{"grad_" + n: v.grad for n, v in t.items()})
            print(f"{tag}: done", flush=True)
    print(f"{count} arrays in {args.out_dir} from {_C.library_path()}")


if __name__ == "__main__":
    main()
