"""Cost of the median-depth and per-pixel index maps (include/gsr_median.h, GaussianRasterizer(depth_alpha=..., median_depth=True,
index_maps=...)) at a bench.py configuration:

  (a) through gsr_profile_*: median_forward against render_forward of the same step (the same walk with three colour accumulators),
      and median_backward against render_backward -- with the early exit, and with it switched off (GSR_DEBUG_MEDIAN_FULL_WALK);
  (b) the whole depth_alpha step -- forward and backward of colour, depth and alpha, every input requiring a gradient -- without the
      feature, with median_depth=True in the loss, and with the three index maps on top.  Wall time between two events on the stream,
      the three alternated step by step; medians;
  (c) with --parent-library: bench.py's default step (--gpus 1) with this tree's library against the parent commit's, a fresh
      process each, alternated this / parent / this / parent; the default path launches none of the new code, so the two libraries
      are expected to differ by no more than the parent's own two runs do.

One JSON line, printed and appended to profiles/median_bench.jsonl.

    python tools/median_bench.py --config C3 --steps 20 --warmup 3 [--parent-library libgsr_hip_parent.so]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "gaussian-splatting_cc-comments_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def bench_default_step(library, steps, warmup, config):
    """one fresh bench.py process -> ms per step"""
    cmd = [sys.executable, os.path.join(R, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--config", config]
    if library:
        cmd += ["--library", library]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, check=True).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])["ms_per_step"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--mode", default="depth", choices=["depth", "invdepth"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-library", default=None, help="the parent commit's libgsr_hip.so: adds measurement (c)")
    ap.add_argument("--bench-steps", type=int, default=200, help="(c): bench.py --steps")
    ap.add_argument("--bench-warmup", type=int, default=20, help="(c): bench.py --warmup")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "median_bench.jsonl"))
    ap.add_argument("--library", help="another build of the C ABI for every measurement of this process (_C.use_library)")
    args = ap.parse_args()

    c = None
    if args.parent_library:   # first, before this process opens the device: one process on it at a time
        runs = {"this": [], "parent": []}
        for _ in range(2):
            runs["this"].append(bench_default_step(None, args.bench_steps, args.bench_warmup, args.config))
            runs["parent"].append(bench_default_step(os.path.abspath(args.parent_library), args.bench_steps, args.bench_warmup, args.config))
        spread = abs(runs["parent"][0] - runs["parent"][1])
        diff = statistics.mean(runs["this"]) - statistics.mean(runs["parent"])
        c = {"bench_steps": args.bench_steps, "bench_warmup": args.bench_warmup, "this_ms": runs["this"], "parent_ms": runs["parent"], "parent_spread_ms": round(spread, 4), "this_minus_parent_ms": round(diff, 4),
             "within_parent_spread": bool(abs(diff) <= spread)}

    import torch

    import gsr_scene
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C
    if args.library:
        _C.use_library(args.library)
    dev = torch.device("cuda:0")
    scene, cam, D = gsr_scene.make_config(args.config, seed=0)
    H, W, P = cam.image_height, cam.image_width, int(scene.means3D.size(0))
    to = lambda t: t.to(dev).contiguous()
    st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=to(scene.bg),
                                       scale_modifier=1.0, viewmatrix=to(cam.world_view_transform), projmatrix=to(cam.full_proj_transform),
                                       sh_degree=D, campos=to(cam.camera_center), prefiltered=False, debug=False)
    st_full = st._replace(debug=_C.DEBUG_MEDIAN_FULL_WALK)   # the same step with the early exit switched off
    leaf = lambda t: to(t).requires_grad_(True)
    t = dict(means3D=leaf(scene.means3D), shs=leaf(scene.shs), opacities=leaf(scene.opacities), scales=leaf(scene.scales),
             rotations=leaf(scene.rotations))
    t["means2D"] = torch.zeros(P, 3, device=dev, requires_grad=True)
    gen = torch.Generator().manual_seed(1)
    dpix = to(torch.randn(3, H, W, generator=gen))
    g, dD, dA = (to(torch.randn(1, H, W, generator=gen)) for _ in range(3))
    maps = (torch.empty(H, W, dtype=torch.int32, device=dev), torch.empty(H, W, dtype=torch.int32, device=dev),
            torch.empty(H, W, dtype=torch.float32, device=dev))

    def clear():
        for v in t.values():
            v.grad = None

    def step_median(settings=st, index_maps=None):
        color, radii, depth, alpha, med = GaussianRasterizer(settings, depth_alpha=args.mode, median_depth=True, index_maps=index_maps)(**t)
        ((color * dpix).sum() + (depth * dD).sum() + (alpha * dA).sum() + (med * g).sum()).backward()

    def step_plain():
        color, radii, depth, alpha = GaussianRasterizer(st, depth_alpha=args.mode)(**t)
        ((color * dpix).sum() + (depth * dD).sum() + (alpha * dA).sum()).backward()

    wall = {"median": [], "median_and_maps": [], "plain": []}
    stages = {"exit": {}, "full_walk": {}}
    for it in range(args.warmup + args.steps):
        for name, f in (("median", step_median), ("median_and_maps", lambda: step_median(index_maps=maps)), ("plain", step_plain)):
            clear()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize(dev)
            if it >= args.warmup:
                wall[name].append(e0.elapsed_time(e1))
        # the stages, recorded in steps of their own (event pairs around every stage cost the step time)
        for key, settings in (("exit", st), ("full_walk", st_full)):
            clear()
            _C.profile_begin(device=dev)
            step_median(settings, maps)
            for name, ms in _C.profile_end(device=dev):
                if it >= args.warmup:
                    stages[key].setdefault(name, []).append(ms)
    med = {k: {n: statistics.median(v) for n, v in s.items()} for k, s in stages.items()}
    new, both, plain = (statistics.median(wall[k]) for k in ("median", "median_and_maps", "plain"))

    def a_of(m):
        return {"median_forward": round(m["median_forward"], 4), "render_forward": round(m["render_forward"], 4),
                "forward_over_render_forward": round(m["median_forward"] / m["render_forward"], 3),
                "median_backward": round(m["median_backward"], 4), "render_backward": round(m["render_backward"], 4),
                "backward_over_render_backward": round(m["median_backward"] / m["render_backward"], 3)}
    out = {"library": _C.library_path(), "config": args.config, "mode": args.mode, "P": P, "W": W, "H": H, "steps": args.steps, "warmup": args.warmup,
           "a_stages_ms": a_of(med["exit"]), "a_stages_full_walk_ms": a_of(med["full_walk"]),
           "b_step_ms": {"plain_depth_alpha": round(plain, 4), "with_median_depth": round(new, 4), "with_median_depth_and_index_maps": round(both, 4),
                         "ratio_to_plain": round(new / plain, 3), "added_over_plain_ms": round(new - plain, 4),
                         "index_maps_added_ms": round(both - new, 4)}}
    if c is not None:
        out["c_default_step_ms"] = c
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
