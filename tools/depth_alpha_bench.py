"""Cost of the depth and alpha maps (GaussianRasterizer(..., depth_alpha=...)) in a forward + backward step, three ways:

  (a) default        image only
  (b) depth_alpha    image + D + A from the same blend pass, random dL/dD and dL/dA
  (c) two passes     the workaround: a second full rasterizer call with colors_precomp = (v, 1, 0) on a black background

Device events around each step after warm-up; the three are alternated in one process (a b c a b c ...) so that clock and
thermal drift fall on all of them alike.  Prints one JSON line per configuration.

    python tools/depth_alpha_bench.py --config C3 --steps 30 --warmup 5 [--mode depth|invdepth]
"""
import argparse
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "gaussian-splatting_cc-comments_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch  # noqa: E402

import gsr_scene  # noqa: E402
from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=["C1", "C2", "C3", "C5"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mode", default="depth", choices=["depth", "invdepth"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for cfg in args.config or ["C3", "C5"]:
        scene, cam, D = gsr_scene.make_config(cfg, seed=0)
        H, W = cam.image_height, cam.image_width
        st = GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=scene.bg.to(dev), scale_modifier=1.0,
            viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev), sh_degree=D,
            campos=cam.camera_center.to(dev), prefiltered=False, debug=False)
        st0 = st._replace(bg=torch.zeros(3, device=dev))
        leaf = {k: getattr(scene, k).to(dev).requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
        means2D = torch.zeros_like(leaf["means3D"], requires_grad=True)
        g = torch.Generator(device=dev).manual_seed(1)
        dpix = torch.randn(3, H, W, device=dev, generator=g)
        dD = torch.randn(1, H, W, device=dev, generator=g)
        dA = torch.randn(1, H, W, device=dev, generator=g)
        plain, aux = GaussianRasterizer(st), GaussianRasterizer(st, depth_alpha=args.mode)
        black = GaussianRasterizer(st0)
        V = st.viewmatrix

        def step_a():
            c, _ = plain(means2D=means2D, **leaf)
            (c * dpix).sum().backward()

        def step_b():
            c, _, d, a = aux(means2D=means2D, **leaf)
            ((c * dpix).sum() + (d * dD).sum() + (a * dA).sum()).backward()

        def step_c():
            c, _ = plain(means2D=means2D, **leaf)
            z = leaf["means3D"] @ V[:3, 2] + V[3, 2]
            v = z if args.mode == "depth" else 1.0 / z
            cols = torch.stack([v, torch.ones_like(v), torch.zeros_like(v)], 1)
            x, _ = black(means3D=leaf["means3D"], means2D=means2D, colors_precomp=cols, opacities=leaf["opacities"],
                         scales=leaf["scales"], rotations=leaf["rotations"])
            ((c * dpix).sum() + (x[0] * dD[0]).sum() + (x[1] * dA[0]).sum()).backward()

        steps = {"a_default": step_a, "b_depth_alpha": step_b, "c_two_pass": step_c}
        times = {k: [] for k in steps}
        for it in range(args.warmup + args.steps):
            for k, f in steps.items():
                for t in list(leaf.values()) + [means2D]:
                    t.grad = None
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                if it >= args.warmup:
                    times[k].append(e0.elapsed_time(e1))
        med = {k: statistics.median(v) for k, v in times.items()}
        out = {"config": cfg, "mode": args.mode, "steps": args.steps, "warmup": args.warmup,
               "median_ms": {k: round(v, 4) for k, v in med.items()},
               "min_ms": {k: round(min(v), 4) for k, v in times.items()},
               "ratio_b_over_a": round(med["b_depth_alpha"] / med["a_default"], 3),
               "ratio_c_over_a": round(med["c_two_pass"] / med["a_default"], 3)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
