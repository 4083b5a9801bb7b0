"""Cost of TSDF fusion and mesh extraction (include/gsr_tsdf.h, fused_tsdf.py) against their floors and against the stock-PyTorch fp32
sequence a user writes, on the same GPU:

  (i)  integration of 200 views of 1980 x 1080 (depth and colour) into 256^3 and 512^3, cameras on a sphere around the volume looking at
       its centre (and, beside it, near the centre looking outward: each then sees a sixth of the volume), the depth maps those of
       an analytic sphere: the batched kernel against
         - the stock per-view sequence (project every node, grid_sample(nearest) of the depth and the colour, masked update of the
           five planes), timed over --stock-views views and scaled to the batch;
         - the floor, the larger of the planes' bytes once in and once out (40 B a node) over 8 TB/s and the vector-ALU time of the
           node-camera pairs: the instructions of the kernel's camera loop up to the depth test (PAIR_LOOP, read off the gfx950 ISA of
           csrc/tsdf.hip) at the fastest rate tools/valu_probe.hip recorded for a mix;
  (ii) extraction of a sphere crossing those grids: plan (with its read-back) and emit, against the planes read once (8 B a node), the
       scratch written and read (5 B a node each way) and the outputs (24 B a vertex with colours, 12 B a face) over 8 TB/s.  Stock
       PyTorch has no extraction step.

Every fused call goes straight to the C entry point with buffers allocated beforehand; wall time between two events on the stream,
medians.  Every step (one grid, one of the two parts) runs in a process of its own under its own time limit, and the whole series
runs --processes times, one after the other; a step that fails or runs out of time ends the series.  One JSON line per step, printed
and appended to profiles/tsdf_bench.jsonl.

    python tools/tsdf_bench.py --steps 5 --warmup 1
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "gaussian-splatting_cc-comments_amd"), os.path.join(R, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_BYTES_PER_S = 8e12
MIX_RATE = 880e9          # wave-instructions per second of the whole chip, the fastest mix of tools/valu_probe.hip
# the camera loop per node-camera pair, from the gfx950 ISA of gsr_tsdf_integrate_kernel<true, false>: the block every pair runs, from
# the record's loads to the -sdf_trunc cut, holds 41 vector instructions (three fma chains, the reciprocal, U and V, the comparisons,
# the pixel's address, the depth and weight tests), one of them the quarter-rate reciprocal, counted as 4: 44.  (A pair that adds to
# the sums runs 12 more; the block's 42 scalar instructions -- the record's loads, the masks of the skips -- issue beside the vector ones.)
PAIR_LOOP = 44


def ring(C, centre, radius, W, H, f, outward=False):
    """C cameras on a spiral over the sphere of `radius` around `centre`, looking at it (outward: away from it) -> packed (C, 20) records
    on the host"""
    import numpy as np
    import torch
    import torch_tsdf as ref
    rec = []
    for c in range(C):
        z = 0.8 * (2.0 * (c + 0.5) / C - 1.0)
        ang = c * math.pi * (3.0 - math.sqrt(5.0))
        s = math.sqrt(1.0 - z * z)
        pos = [centre[0] + radius * s * math.cos(ang), centre[1] + radius * z, centre[2] + radius * s * math.sin(ang)]
        rec.append(ref.look_at(pos, [2.0 * a - b for a, b in zip(pos, centre)] if outward else centre, W, H, f))
    return torch.from_numpy(np.stack(rec))


def sphere_depth(rec, centre, r, H, W, dev, torch, far=False):
    """z-depth of the sphere (centre, r) at pixel centres for every record (far: its far side, for a camera inside it), 0 where the ray
    misses -> (C, H, W) float32 on dev"""
    out = torch.empty((rec.shape[0], H, W), dtype=torch.float32, device=dev)
    vv, uu = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32) + 0.5, torch.arange(W, device=dev, dtype=torch.float32) + 0.5, indexing="ij")
    cen = torch.tensor(centre, dtype=torch.float32, device=dev)
    for c in range(rec.shape[0]):
        k = rec[c].to(dev)
        Rm, t = k[:9].reshape(3, 3), k[9:12]
        o = -(Rm.T @ t) - cen
        d = torch.stack([(uu - k[14]) / k[12], (vv - k[15]) / k[13], torch.ones_like(uu)], dim=-1) @ Rm
        a, b, cc = (d * d).sum(-1), 2.0 * (d @ o), float(o @ o) - r * r
        disc = b * b - 4 * a * cc
        out[c] = torch.where(disc > 0, (-b + (1.0 if far else -1.0) * disc.clamp(min=0).sqrt()) / (2 * a), torch.zeros_like(a))
    return out


def stock_view(torch, xyz, wsum, dsum, csum, k, depth, color, trunc):
    """one view of the sequence a user writes with stock PyTorch (the per-view form of 2DGS's extract_mesh_unbounded): fp32, whole grid"""
    Rm, t = k[:9].reshape(3, 3), k[9:12]
    p = xyz @ Rm.T + t
    z = p[:, 2]
    H, W = depth.shape
    u = p[:, 0] / z * k[12] + k[14]
    v = p[:, 1] / z * k[13] + k[15]
    grid = torch.stack([u / W * 2.0 - 1.0, v / H * 2.0 - 1.0], dim=-1)[None, None]
    d = torch.nn.functional.grid_sample(depth[None, None], grid, mode="nearest", padding_mode="zeros", align_corners=False)[0, 0, 0]
    rgb = torch.nn.functional.grid_sample(color[None], grid, mode="nearest", padding_mode="zeros", align_corners=False)[0, :, 0]
    sdf = d - z
    mask = (z > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H) & (d > 0) & (sdf >= -trunc)
    w = mask.float()
    wsum += w
    dsum += w * (sdf / trunc).clamp(max=1.0)
    csum += w[None] * rgb


def child(args):
    import torch

    import fused_tsdf as ft
    from diff_gaussian_rasterization import _C
    if args.library:
        _C.use_library(os.path.abspath(args.library))
    dev = torch.device("cuda:0")
    lib = ft._lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    part, n = args.child.split(":")
    n = int(n)
    nodes = n ** 3

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def medians(runs, steps, warmup):
        ms = {k: [] for k in runs}
        names = list(runs)
        for it in range(warmup + steps):
            for k in names[it % len(names):] + names[:it % len(names)]:   # rotated: no candidate always runs behind the same one
                t = timed(runs[k])
                if it >= warmup:
                    ms[k].append(t)
        return {k: statistics.median(v) for k, v in ms.items()}

    def check(rc):
        assert rc == 0, lib.gsr_last_error()

    half, radius = 1.0, 0.7
    vs = 2.0 * half / (n - 1)
    grid = ft.Grid(n, n, n, (ctypes.c_float * 3)(-half, -half, -half), vs)
    out = {"part": part, "grid": n, "steps": args.steps, "warmup": args.warmup, "library": os.path.basename(args.library) if args.library else None}
    if part == "integrate":
        C, W, H = args.views, args.width, args.height
        color = torch.rand((C, 3, H, W), device=dev)
        trunc = 4.0 * vs
        planes = (torch.zeros(nodes, device=dev), torch.zeros(nodes, device=dev), torch.zeros(3, nodes, device=dev))
        zero_ms = medians({"zero": lambda: [t.zero_() for t in planes]}, args.steps, 1)["zero"]
        layouts = {}
        # "around": the object-centred capture, every camera sees the whole volume.  "inside": a scene-scale capture, the cameras near the
        # centre looking outward at the sphere's inner side, each seeing about a sixth of the volume
        for layout in ("around", "inside"):
            inside = layout == "inside"
            rec_host = ring(C, (0.0, 0.0, 0.0), 0.2 if inside else 4.0, W, H, 0.5 * H * (1.0 if inside else 4.0 / (1.5 * half)), inside).contiguous()
            rec = rec_host.to(dev)
            depth = sphere_depth(rec_host, (0.0, 0.0, 0.0), radius, H, W, dev, torch, far=inside)

            def fused():
                w, d, c = planes
                w.zero_(); d.zero_(); c.zero_()
                check(lib.gsr_tsdf_integrate(ctypes.byref(grid), w.data_ptr(), d.data_ptr(), c.data_ptr(), C, rec.data_ptr(), rec_host.data_ptr(), H, W,
                                             depth.data_ptr(), color.data_ptr(), None, trunc, math.inf, stream))

            med = medians({"fused": fused}, args.steps, args.warmup)
            first = [t.clone() for t in planes[:2]]
            fused()
            same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, planes))
            layouts[layout] = {"ms": round(med["fused"] - zero_ms, 3), "same_bits_on_a_second_run": same, "nodes_touched": int((planes[0] > 0).sum()),
                               "mean_views_per_touched_node": round(float(planes[0].sum()) / max(1, int((planes[0] > 0).sum())), 1)}
        fused_ms = layouts["around"]["ms"]
        # the stock sequence over a few views, on planes of its own
        k, j, i = torch.meshgrid(*(torch.arange(n, device=dev, dtype=torch.float32),) * 3, indexing="ij")
        xyz = torch.stack([i.reshape(-1), j.reshape(-1), k.reshape(-1)], dim=1) * vs - half
        del i, j, k
        sw, sd, sc = torch.zeros(nodes, device=dev), torch.zeros(nodes, device=dev), torch.zeros(3, nodes, device=dev)
        views = min(args.stock_views, C)

        def stock():
            for c in range(views):
                stock_view(torch, xyz, sw, sd, sc, rec[c], depth[c], color[c], trunc)

        stock_ms = medians({"stock": stock}, max(1, args.steps // 2), 1)["stock"] * C / views
        bytes_ms = nodes * 40 / HBM_BYTES_PER_S * 1e3
        valu_ms = (nodes / 64.0) * C * PAIR_LOOP / MIX_RATE * 1e3
        floor = max(bytes_ms, valu_ms)
        out.update({"views": C, "image": [W, H], "i_fused": layouts, "zeroing_ms_subtracted": round(zero_ms, 3), "i_stock_pytorch_ms": round(stock_ms, 1), "stock_views_timed": views,
                    "i_stock_over_fused": round(stock_ms / fused_ms, 1), "bytes_floor_ms": round(bytes_ms, 3),
                    "valu_floor_ms": round(valu_ms, 3), "fused_over_floor": round(fused_ms / floor, 2),
                    "pair_loop_instructions": PAIR_LOOP})
    else:
        k, j, i = torch.meshgrid(*(torch.arange(n, device=dev, dtype=torch.float32),) * 3, indexing="ij")
        x, y, z = i * vs - half + 0.013, j * vs - half - 0.007, k * vs - half + 0.004   # the field's centre lies off the grid's
        del i, j, k
        wsum = 1.0 + 2.0 * torch.rand((n, n, n), device=dev)
        dsum = wsum * ((x * x + y * y + z * z).sqrt() - radius)
        csum = torch.stack([wsum * (0.5 + 0.5 * torch.sin(3.0 * x)), wsum * (0.5 + 0.5 * torch.cos(2.0 * y)), wsum * 0.5]).contiguous()
        del x, y, z
        scratch = torch.empty(lib.gsr_tsdf_mesh_scratch_bytes(nodes), dtype=torch.uint8, device=dev)
        plan = ft.MeshPlan()

        def do_plan():
            check(lib.gsr_tsdf_mesh_plan(ctypes.byref(grid), wsum.data_ptr(), dsum.data_ptr(), 1.0, scratch.data_ptr(), ctypes.byref(plan), stream))

        do_plan()
        V, F = int(plan.V), int(plan.F)
        vert, cols, faces = torch.empty((V, 3), device=dev), torch.empty((V, 3), device=dev), torch.empty((F, 3), dtype=torch.int32, device=dev)

        def do_emit():
            check(lib.gsr_tsdf_mesh_emit(ctypes.byref(plan), V, F, csum.data_ptr(), vert.data_ptr(), cols.data_ptr(), faces.data_ptr(), stream))

        med = medians({"plan": do_plan, "emit": do_emit}, args.steps, args.warmup)
        first = (vert.clone(), faces.clone())
        do_plan(); do_emit()
        torch.cuda.synchronize(dev)
        off = vert + torch.tensor([0.013, -0.007, 0.004], device=dev)
        err = float(((off * off).sum(dim=1).sqrt() - radius).abs().max() / vs)
        floor_ms = (nodes * (8 + 10) + V * 24 + F * 12) / HBM_BYTES_PER_S * 1e3
        out.update({"V": V, "F": F, "ii_plan_ms": round(med["plan"], 3), "ii_emit_ms": round(med["emit"], 3),
                    "ii_extract_ms": round(med["plan"] + med["emit"], 3), "bytes_floor_ms": round(floor_ms, 3),
                    "extract_over_floor": round((med["plan"] + med["emit"]) / floor_ms, 2),
                    "same_bits_on_a_second_run": bool(torch.equal(first[0], vert) and torch.equal(first[1], faces)),
                    "largest_distance_to_the_sphere_in_voxels": round(err, 4)})
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--grids", default="256,512")
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--width", type=int, default=1980)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--stock-views", type=int, default=8)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds one step (one grid, one part, one process) may take")
    ap.add_argument("--library", default=None, help="a variant build of libgsr_hip.so (csrc/Makefile, `make variant`) to run instead")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "tsdf_bench.jsonl"))
    ap.add_argument("--child", default=None, help="measure this step in this process: integrate:N or mesh:N (what the tool starts)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    passed = [a for a in sys.argv[1:]]
    for _ in range(args.processes):   # fresh processes, one after the other; this one never opens the device
        for n in args.grids.split(","):
            for part in ("integrate", "mesh"):
                # a step that fails or runs out of time raises here: nothing more is started on the device
                subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{part}:{int(n)}"] + passed, check=True, timeout=args.step_timeout)


if __name__ == "__main__":
    main()
