"""Cost of the absolute screen-space gradients (GaussianRasterizer(..., absgrad=(abs_mean2D, abs_gradient_accum))) in a forward +
backward step:

  (a) default   the step as it is without the keyword
  (b) absgrad   the same step with both tensors given: the ABS backward blend and the fold pass behind it

Device events around each step after warm-up; the two are alternated in one process (a b a b ...) so that clock and thermal drift
fall on both alike.  After the timed steps one more step of each runs under the library's stage profile and the backward blend's
time (`render_backward`) and the fold kernel's (`absgrad_fold`) are reported.  Prints one JSON line per configuration.

    python tools/absgrad_bench.py --config C3 --steps 20 --warmup 5
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
from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=["C1", "C2", "C3", "C5"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for cfg in args.config or ["C3", "C5"]:
        scene, cam, D = gsr_scene.make_config(cfg, seed=0)
        H, W = cam.image_height, cam.image_width
        cams = [t.to(dev) for t in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)]
        st = GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=scene.bg.to(dev), scale_modifier=1.0,
            viewmatrix=cams[0], projmatrix=cams[1], sh_degree=D, campos=cams[2], prefiltered=False, debug=False)
        leaf = {k: getattr(scene, k).to(dev).requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
        means2D = torch.zeros_like(leaf["means3D"], requires_grad=True)
        dpix = torch.randn(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        P = leaf["means3D"].shape[0]
        absgrad = (torch.empty(P, 2, device=dev), torch.zeros(P, device=dev))
        rast = {"a_default": GaussianRasterizer(st), "b_absgrad": GaussianRasterizer(st, absgrad=absgrad)}

        def step(k):
            for t in list(leaf.values()) + [means2D]:
                t.grad = None
            c, _ = rast[k](means2D=means2D, **leaf)
            (c * dpix).sum().backward()

        times = {k: [] for k in rast}
        for it in range(args.warmup + args.steps):
            for k in rast:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(k)
                e1.record()
                e1.synchronize()
                if it >= args.warmup:
                    times[k].append(e0.elapsed_time(e1))
        stages = {}
        for k in rast:
            _C.profile_begin(device=dev)
            step(k)
            torch.cuda.synchronize()
            prof = _C.profile_end(device=dev)
            stages[k] = {n: round(sum(ms for name, ms in prof if name == n), 4) for n in ("render_backward", "absgrad_fold", "gaussian_backward")}
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps({"config": cfg, "steps": args.steps, "warmup": args.warmup,
                          "median_ms": {k: round(v, 4) for k, v in med.items()},
                          "min_ms": {k: round(min(v), 4) for k, v in times.items()},
                          "ratio_b_over_a": round(med["b_absgrad"] / med["a_default"], 3),
                          "stage_ms": stages}), flush=True)


if __name__ == "__main__":
    main()
