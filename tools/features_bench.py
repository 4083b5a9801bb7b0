"""Cost of K blended feature channels (include/gsr_features.h, GaussianRasterizer.forward(features=...)) at a bench.py configuration:

  (a) per chunk of four channels, through gsr_profile_*: the forward tile pass against render_forward of the same step (the same walk
      with three accumulators: the floor), and the backward tile pass against render_backward;
  (b) the whole step -- forward and backward of colour plus K channels, every input requiring a gradient -- against what a user had
      before: 1 + ceil(K / 3) rasterizer calls, the extra ones with colors_precomp = three channels on a zero background.  Wall time
      between two events on the stream, the two alternated step by step; medians.

One JSON line per K, printed and appended to profiles/features_bench.jsonl.

    python tools/features_bench.py --config C3 --K 4 --K 16 --steps 20 --warmup 3
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
    ap.add_argument("--config", default="C3", choices=list(gsr_scene.CONFIGS))
    ap.add_argument("--K", type=int, action="append")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "features_bench.jsonl"))
    ap.add_argument("--library", help="another build of the C ABI for every measurement of this process (_C.use_library)")
    args = ap.parse_args()
    if args.library:
        _C.use_library(args.library)
    dev = torch.device("cuda:0")
    scene, cam, D = gsr_scene.make_config(args.config, seed=0)
    H, W, P = cam.image_height, cam.image_width, int(scene.means3D.size(0))
    to = lambda t: t.to(dev).contiguous()
    st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=to(scene.bg),
                                       scale_modifier=1.0, viewmatrix=to(cam.world_view_transform), projmatrix=to(cam.full_proj_transform),
                                       sh_degree=D, campos=to(cam.camera_center), prefiltered=False, debug=False)
    st0 = st._replace(bg=torch.zeros(3, device=dev))
    leaf = lambda t: to(t).requires_grad_(True)
    t = dict(means3D=leaf(scene.means3D), shs=leaf(scene.shs), opacities=leaf(scene.opacities), scales=leaf(scene.scales),
             rotations=leaf(scene.rotations))
    t["means2D"] = torch.zeros(P, 3, device=dev, requires_grad=True)
    geo = {k: t[k] for k in ("means3D", "means2D", "opacities", "scales", "rotations")}
    gen = torch.Generator().manual_seed(1)
    dpix = to(torch.randn(3, H, W, generator=gen))

    for K in args.K or [4, 16]:
        feats = to(torch.randn(P, K, generator=gen)).requires_grad_(True)
        g = to(torch.randn(K, H, W, generator=gen))
        nchunks = (K + 3) // 4
        npass = (K + 2) // 3

        def clear():
            for v in list(t.values()) + [feats]:
                v.grad = None

        def step_new():
            color, radii, fmap = GaussianRasterizer(st)(**t, features=feats)
            ((color * dpix).sum() + (fmap * g).sum()).backward()

        def step_old():
            color, _ = GaussianRasterizer(st)(**t)
            loss = (color * dpix).sum()
            for k0 in range(0, K, 3):
                n = min(3, K - k0)
                cols = torch.cat([feats[:, k0:k0 + n], torch.zeros(P, 3 - n, device=dev)], 1)
                m, _ = GaussianRasterizer(st0)(colors_precomp=cols, **geo)
                loss = loss + (m[:n] * g[k0:k0 + n]).sum()
            loss.backward()

        wall = {"new": [], "old": []}
        stages = {}
        for it in range(args.warmup + args.steps):
            for name, f in (("new", step_new), ("old", step_old)):
                clear()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize(dev)
                if it >= args.warmup:
                    wall[name].append(e0.elapsed_time(e1))
            # the stages of the new step, recorded in a step of their own (event pairs around every stage cost the step time)
            clear()
            _C.profile_begin(device=dev)
            step_new()
            for name, ms in _C.profile_end(device=dev):
                if it >= args.warmup:
                    stages.setdefault(name, []).append(ms)
        med = {n: statistics.median(v) for n, v in stages.items()}
        new, old = statistics.median(wall["new"]), statistics.median(wall["old"])
        out = {"library": _C.library_path(), "config": args.config, "P": P, "W": W, "H": H, "K": K, "chunks": nchunks, "steps": args.steps, "warmup": args.warmup,
               "a_forward_ms": {"features_forward": round(med["features_forward"], 4), "per_chunk": round(med["features_forward"] / nchunks, 4),
                                "render_forward": round(med["render_forward"], 4),
                                "per_chunk_over_render_forward": round(med["features_forward"] / nchunks / med["render_forward"], 3)},
               "a_backward_ms": {"features_backward_tiles": round(med["features_backward_tiles"], 4),
                                 "per_chunk": round(med["features_backward_tiles"] / nchunks, 4),
                                 "features_backward_fold": round(med["features_backward_fold"], 4),
                                 "render_backward": round(med["render_backward"], 4),
                                 "per_chunk_over_render_backward": round(med["features_backward_tiles"] / nchunks / med["render_backward"], 3)},
               "b_step_ms": {"colour_plus_features": round(new, 4), "alternative": round(old, 4), "alternative_calls": 1 + npass,
                             "ratio": round(new / old, 3), "beats_alternative": bool(new < old)}}
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
