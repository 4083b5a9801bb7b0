"""Cost of the camera gradients under a camera model (GaussianRasterizer(..., camera_model=, camera_model_grads=)) in a forward +
backward step against the plain camera-model step, and the times of the per-Gaussian backward and of the fold behind it (stages
"gaussian_backward" and "camera_grad"):

  pinhole / fisheye                the camera-model step as it was (no keyword)
  pinhole_grads / fisheye_grads    camera_model_grads=True: viewmatrix and campos require a gradient
  pinhole_tensor / fisheye_tensor  camera_model_grads=the (4,) intrinsics tensor, which requires a gradient too

Device events around each step after warm-up; the configurations are alternated in one process (a b c ... a b c ...) so that clock
and thermal drift fall on all alike.  Prints one JSON line per scene configuration.

The baseline of the ratios is the plain camera-model step of ANOTHER build of the library -- the parent commit's -- on the same scene
in a process of its own, never the new code against itself: run once with --library PATH --plain-only (that build has no
camera_model_grads; only the first two are measured) and keep the line, then run the product with --baseline FILE, which adds the
ratio of every median over that file's step with the same model.  The spread between two such baseline runs is the margin.

    python tools/cam_cm_bench.py --library libgsr_hip_parent.so --plain-only --config C3 > parent.jsonl
    python tools/cam_cm_bench.py --baseline parent.jsonl --config C3 --steps 30 --warmup 5
"""
import argparse
import json
import math
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

KERNELS = ("gaussian_backward", "camera_grad")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=["C1", "C2", "C3", "C5"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--library", help="another build of the C ABI to bind instead of the product library")
    ap.add_argument("--plain-only", action="store_true", help="measure the plain camera-model steps alone: a library without camera_model_grads")
    ap.add_argument("--baseline", help="JSON lines of a --plain-only run of the parent commit's library")
    args = ap.parse_args()
    if args.library:
        _C.use_library(args.library)
    baseline = {}
    if args.baseline:
        for line in open(args.baseline):
            if line.startswith("{"):
                rec = json.loads(line)
                baseline[rec["config"]] = rec
    dev = torch.device("cuda:0")
    for cfg in args.config or ["C3"]:
        scene, cam, D = gsr_scene.make_config(cfg, seed=0)
        H, W = cam.image_height, cam.image_width
        cams = [cam.world_view_transform.to(dev).requires_grad_(True), cam.camera_center.to(dev).requires_grad_(True)]
        st = GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=scene.bg.to(dev), scale_modifier=1.0,
            viewmatrix=cams[0], projmatrix=cam.full_proj_transform.to(dev), sh_degree=D, campos=cams[1], prefiltered=False, debug=False)
        leaf = {k: getattr(scene, k).to(dev).requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
        means2D = torch.zeros_like(leaf["means3D"], requires_grad=True)
        dpix = torch.randn(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        fx, fy = W / (2.0 * cam.tanfovx), H / (2.0 * cam.tanfovy)
        f_eq = (W / 2.0) / math.atan(cam.tanfovx)   # equidistant: the same horizontal field of view reaches the image edge
        models = {"pinhole": ("pinhole", fx, fy, W / 2.0, H / 2.0), "fisheye": ("fisheye", f_eq, f_eq, W / 2.0, H / 2.0)}
        rasterizers, handles = {}, []
        for name, cm in models.items():
            rasterizers[name] = GaussianRasterizer(st, camera_model=cm)
        if not args.plain_only:
            for name, cm in models.items():
                rasterizers[name + "_grads"] = GaussianRasterizer(st, camera_model=cm, camera_model_grads=True)
            for name, cm in models.items():
                k = torch.tensor([float(v) for v in cm[1:]], device=dev, requires_grad=True)
                handles.append(k)
                rasterizers[name + "_tensor"] = GaussianRasterizer(st, camera_model=cm, camera_model_grads=k)

        def step(r):
            c, _ = r(means2D=means2D, **leaf)
            (c * dpix).sum().backward()

        def clear():
            for t in list(leaf.values()) + [means2D] + cams + handles:
                t.grad = None

        times = {k: [] for k in rasterizers}
        for it in range(args.warmup + args.steps):
            for k, r in rasterizers.items():
                clear()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(r)
                e1.record()
                e1.synchronize()
                if it >= args.warmup:
                    times[k].append(e0.elapsed_time(e1))
        # the per-Gaussian backward and the fold, one recorded alone per step (recording every stage serialises the forward's streams)
        kernel_ms = {k: {} for k in rasterizers}
        for k, r in rasterizers.items():
            for name in KERNELS:
                vals = []
                for _ in range(max(3, args.steps // 3)):
                    clear()
                    _C.profile_begin(only=name, device=dev)
                    step(r)
                    torch.cuda.synchronize()
                    vals += [ms for n, ms in _C.profile_end(device=dev) if n == name]
                kernel_ms[k][name] = round(statistics.median(vals), 5) if vals else None
        med = {k: statistics.median(v) for k, v in times.items()}
        out = {"config": cfg, "steps": args.steps, "warmup": args.warmup, "library": os.path.basename(_C.library_path()),
               "median_ms": {k: round(v, 4) for k, v in med.items()},
               "min_ms": {k: round(min(v), 4) for k, v in times.items()},
               "kernel_ms": kernel_ms}
        if cfg in baseline:
            base = baseline[cfg]
            model_of = lambda k: k.split("_")[0]
            out["baseline_library"] = base.get("library")
            out["baseline_median_ms"] = {m: base["median_ms"][m] for m in models}
            out["ratio_over_baseline"] = {k: round(v / base["median_ms"][model_of(k)], 3) for k, v in med.items()}
            out["gaussian_backward_ratio_over_baseline"] = {
                k: (round(ks["gaussian_backward"] / base["kernel_ms"][model_of(k)]["gaussian_backward"], 3)
                    if ks.get("gaussian_backward") and base["kernel_ms"][model_of(k)].get("gaussian_backward") else None)
                for k, ks in kernel_ms.items()}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
