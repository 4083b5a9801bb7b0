"""Cost of the per-Gaussian blend-weight statistics (include/gsr_contrib.h, _C.gaussian_contributions), per stage through gsr_profile_*:

  (a) the two new stages, contrib_tiles (with the clearing of its validity bytes) and contrib_gaussians, after a forward;
  (b) the render_forward stage of the same step -- the same walk with three accumulators and no per-instance reduction: the floor;
  (c) what a user had to run before: forward with colors_precomp + backward with an all-ones dL/dpix, whose dL/dcolors[:, 0] is the
      weight sum -- its render_backward and gaussian_backward stages (the blend and per-Gaussian translation units are the parent
      commit's, unchanged; --substitute-only times (c) alone, for a run against another build with --library).

Every stage is recorded (event pairs around each), steps alternate (a)+(b) and (c); medians over the steps.  One JSON line per
configuration.

    python tools/contrib_bench.py --config C3 --config C5 --steps 20 --warmup 3
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
from diff_gaussian_rasterization import _C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=["C1", "C2", "C3", "C5"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--library", help="another build of the C ABI (csrc/Makefile `variant`)")
    ap.add_argument("--substitute-only", action="store_true", help="time (c) alone (a build without gsr_contributions)")
    ap.add_argument("--pixel-weight", action="store_true", help="pass a weight map to the pass (default: m = 1)")
    args = ap.parse_args()
    if args.library:
        _C.use_library(args.library)
    dev = torch.device("cuda:0")
    for cfg in args.config or ["C3", "C5"]:
        scene, cam, D = gsr_scene.make_config(cfg, seed=0)
        H, W, P = cam.image_height, cam.image_width, int(scene.means3D.size(0))
        to = lambda t: t.to(dev).contiguous()
        e = torch.empty(0, device=dev)
        bg, means, opac, scales, rots, shs = (to(t) for t in (scene.bg, scene.means3D, scene.opacities, scene.scales, scene.rotations, scene.shs))
        view, proj, campos = to(cam.world_view_transform), to(cam.full_proj_transform), to(cam.camera_center)
        colors = torch.rand(P, 3, device=dev)
        ones = torch.ones(3, H, W, device=dev)
        m = torch.rand(H, W, device=dev) + 0.5 if args.pixel_weight else None
        stats = (torch.zeros(P, device=dev), torch.zeros(P, device=dev), torch.zeros(P, dtype=torch.int32, device=dev))

        def forward(col, sh):
            return _C.rasterize_gaussians(bg, means, col, opac, scales, rots, 1.0, e, view, proj, cam.tanfovx, cam.tanfovy, H, W, sh, D, campos,
                                          False, False)

        def step_new():
            r = forward(e, shs)
            _C.gaussian_contributions(r[3], r[4], r[5], r[0], P, W, H, stats, m)
            return r[0]

        def step_substitute():
            r = forward(colors, e)
            _C.rasterize_gaussians_backward(bg, means, r[2], colors, scales, rots, 1.0, e, view, proj, cam.tanfovx, cam.tanfovy, ones, e, D,
                                            campos, r[3], r[0], r[4], r[5], False, lean=True)
            return r[0]

        steps = {"substitute": step_substitute} if args.substitute_only else {"new": step_new, "substitute": step_substitute}
        times = {k: {} for k in steps}
        rendered = 0
        for it in range(args.warmup + args.steps):
            for k, f in steps.items():
                _C.profile_begin(device=dev)
                rendered = f()
                for name, ms in _C.profile_end(device=dev):
                    if it >= args.warmup:
                        times[k].setdefault(name, []).append(ms)
        med = {k: {n: statistics.median(v) for n, v in t.items()} for k, t in times.items()}
        out = {"config": cfg, "P": P, "W": W, "H": H, "num_rendered": int(rendered), "steps": args.steps, "warmup": args.warmup,
               "pixel_weight": bool(args.pixel_weight), "library": _C.library_path()}
        sub = med["substitute"]
        out["c_substitute_ms"] = {n: round(sub[n], 4) for n in ("render_forward", "render_backward", "gaussian_backward") if n in sub}
        c = sub["render_backward"] + sub["gaussian_backward"]
        out["c_backward_stages_ms"] = round(c, 4)
        if "new" in med:
            new = med["new"]
            a = new["contrib_tiles"] + new["contrib_gaussians"]
            out["a_contrib_ms"] = {"contrib_tiles": round(new["contrib_tiles"], 4), "contrib_gaussians": round(new["contrib_gaussians"], 4), "total": round(a, 4)}
            out["b_render_forward_ms"] = round(new["render_forward"], 4)
            out["ratio_a_over_b"] = round(a / new["render_forward"], 3)
            out["ratio_a_over_c"] = round(a / c, 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
