"""Cost of the normal-consistency pieces (include/gsr_normals.h, fused_geometry.py) at a bench.py configuration:

  (a) the three new stages -- gaussian_normals, depth_normals and normal_consistency_loss, forward plus backward each -- against a
      stock-PyTorch evaluation of the same formulas on the GPU in fp32 (tests/torch_normals.py with dtype=float32), forward plus
      backward.  Wall time between two events on the stream, fused and stock alternated call by call; medians;
  (b) the whole depth_alpha step -- forward and backward of colour, depth and alpha, every input requiring a gradient -- without the
      term, with the normal map as three feature channels and the fused loss on depth / alpha, and with the same term written in
      stock PyTorch; the three alternated step by step; medians;
  (c) with --parent-library: bench.py's default step (--gpus 1) with this tree's library against the parent commit's, a fresh
      process each, alternated this / parent / this / parent; the default path launches none of the new code, so the two libraries
      are expected to differ by no more than the parent's own two runs do.

One JSON line, printed and appended to profiles/normals_bench.jsonl.

    python tools/normals_bench.py --config C3 --steps 20 --warmup 3 [--parent-library libgsr_hip_parent.so]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "gaussian-splatting_cc-comments_amd"), os.path.join(R, "tests")):
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-library", default=None, help="the parent commit's libgsr_hip.so: adds measurement (c)")
    ap.add_argument("--bench-steps", type=int, default=200, help="(c): bench.py --steps")
    ap.add_argument("--bench-warmup", type=int, default=20, help="(c): bench.py --warmup")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "normals_bench.jsonl"))
    args = ap.parse_args()

    c = None
    if args.parent_library:   # first, before this process opens the device: one process on it at a time
        runs = {"this": [], "parent": []}
        for _ in range(2):
            runs["this"].append(bench_default_step(None, args.bench_steps, args.bench_warmup, args.config))
            runs["parent"].append(bench_default_step(os.path.abspath(args.parent_library), args.bench_steps, args.bench_warmup, args.config))
        spread = abs(runs["parent"][0] - runs["parent"][1])
        diff = statistics.mean(runs["this"]) - statistics.mean(runs["parent"])
        c = {"bench_steps": args.bench_steps, "bench_warmup": args.bench_warmup, "this_ms": runs["this"], "parent_ms": runs["parent"],
             "parent_spread_ms": round(spread, 4), "this_minus_parent_ms": round(diff, 4), "within_parent_spread": bool(abs(diff) <= spread)}

    import torch

    import gsr_scene
    import torch_normals as tn
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from fused_geometry import depth_normals, gaussian_normals, normal_consistency_loss
    dev = torch.device("cuda:0")
    scene, cam, D = gsr_scene.make_config(args.config, seed=0)
    H, W, P = cam.image_height, cam.image_width, int(scene.means3D.size(0))
    tanx, tany = cam.tanfovx, cam.tanfovy
    to = lambda t: t.to(dev).contiguous()
    V = to(cam.world_view_transform)
    st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=tanx, tanfovy=tany, bg=to(scene.bg), scale_modifier=1.0,
                                       viewmatrix=V, projmatrix=to(cam.full_proj_transform), sh_degree=D, campos=to(cam.camera_center),
                                       prefiltered=False, debug=False)
    leaf = lambda t: to(t).requires_grad_(True)
    t = dict(means3D=leaf(scene.means3D), shs=leaf(scene.shs), opacities=leaf(scene.opacities), scales=leaf(scene.scales),
             rotations=leaf(scene.rotations))
    t["means2D"] = torch.zeros(P, 3, device=dev, requires_grad=True)
    gen = torch.Generator().manual_seed(1)
    dpix = to(torch.randn(3, H, W, generator=gen))
    dD, dA = (to(torch.randn(1, H, W, generator=gen)) for _ in range(2))
    gP, gN = to(torch.randn(P, 3, generator=gen)), to(torch.randn(3, H, W, generator=gen))

    def clear():
        for v in t.values():
            v.grad = None

    # inputs of the image-sized stages: the depth and alpha maps of one render and a normal map of the right statistics
    with torch.no_grad():
        _, _, depth0, alpha0, nmap0 = GaussianRasterizer(st, depth_alpha="depth")(**t, features=gaussian_normals(
            t["scales"], t["rotations"], t["means3D"], V))
        surf0 = (depth0 / alpha0.clamp_min(1e-3)).contiguous()

    def stage_gaussian(fn):
        q = t["rotations"].detach().requires_grad_(True)
        (fn(t["scales"].detach(), q, t["means3D"].detach(), V) * gP).sum().backward()

    def stage_depth(fn):
        z = surf0.clone().requires_grad_(True)
        (fn(z, tanx, tany) * gN).sum().backward()

    def stage_loss(fn):
        z, n = surf0.clone().requires_grad_(True), nmap0.clone().requires_grad_(True)
        fn(n, z, alpha0, tanx, tany).backward()

    f32 = dict(dtype=torch.float32)
    stages = {"gaussian_normals": (stage_gaussian, gaussian_normals, lambda *a: tn.gaussian_normals(*a, **f32)),
              "depth_normals": (stage_depth, depth_normals, lambda *a: tn.depth_normals(*a, **f32)),
              "normal_consistency_loss": (stage_loss, normal_consistency_loss, lambda *a: tn.normal_consistency_loss(*a, **f32))}

    def step(term):
        feats = {}
        if term is not None:
            feats["features"] = (gaussian_normals if term == "fused" else stages["gaussian_normals"][2])(
                t["scales"], t["rotations"], t["means3D"], V)
        out = GaussianRasterizer(st, depth_alpha="depth")(**t, **feats)
        color, depth, alpha = out[0], out[2], out[3]
        loss = (color * dpix).sum() + (depth * dD).sum() + (alpha * dA).sum()
        if term is not None:
            fn = normal_consistency_loss if term == "fused" else stages["normal_consistency_loss"][2]
            loss = loss + 0.05 * fn(out[4], depth / alpha.detach().clamp_min(1e-3), alpha, tanx, tany)
        loss.backward()

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    a = {name: {"fused": [], "stock": []} for name in stages}
    b = {"plain": [], "fused": [], "stock": []}
    for it in range(args.warmup + args.steps):
        for name, (run, fused, stock) in stages.items():
            for key, fn in (("fused", fused), ("stock", stock)):
                ms = timed(lambda: run(fn))
                if it >= args.warmup:
                    a[name][key].append(ms)
        for key, term in (("plain", None), ("fused", "fused"), ("stock", "stock")):
            clear()
            ms = timed(lambda: step(term))
            if it >= args.warmup:
                b[key].append(ms)
    med = statistics.median
    a_out = {name: {"fused_ms": round(med(v["fused"]), 4), "stock_pytorch_ms": round(med(v["stock"]), 4),
                    "stock_over_fused": round(med(v["stock"]) / med(v["fused"]), 2)} for name, v in a.items()}
    a_out["sum"] = {"fused_ms": round(sum(v["fused_ms"] for v in a_out.values()), 4),
                    "stock_pytorch_ms": round(sum(v["stock_pytorch_ms"] for v in a_out.values()), 4)}
    a_out["sum"]["stock_over_fused"] = round(a_out["sum"]["stock_pytorch_ms"] / a_out["sum"]["fused_ms"], 2)
    plain, fused, stock = (med(b[k]) for k in ("plain", "fused", "stock"))
    out = {"config": args.config, "P": P, "W": W, "H": H, "steps": args.steps, "warmup": args.warmup, "a_stages_fwd_bwd_ms": a_out,
           "b_step_ms": {"plain_depth_alpha": round(plain, 4), "with_normals_and_fused_loss": round(fused, 4),
                         "with_normals_and_stock_pytorch": round(stock, 4), "fused_added_ms": round(fused - plain, 4),
                         "stock_added_ms": round(stock - plain, 4), "fused_ratio_to_plain": round(fused / plain, 3),
                         "stock_ratio_to_plain": round(stock / plain, 3)}}
    if c is not None:
        out["c_default_step_ms"] = c
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
