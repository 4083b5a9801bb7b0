"""Cost of the fused 3D smoothing filter (include/gsr_filter3d.h, fused_filter3d.py) against the stock-PyTorch fp32 sequences a user
writes, on the same GPU in the same process:

  (i)   the camera sweep at 1M and 6M Gaussians with 200 cameras against Mip-Splatting's compute_3D_filter as published (a Python loop
        over the cameras, about 20 elementwise launches each) and against the kernel's vector-ALU floor: the instructions of its inner
        loop per Gaussian-camera pair (SWEEP_LOOP, read off the gfx950 ISA of csrc/filter3d.hip) at the rate tools/valu_probe.hip
        measures for a mix of instruction kinds, with the price per kind beside it;
  (ii)  the filtered activations, forward plus backward, at 1M and 6M against the stock sequence with autograd and against the
        streaming floor of 88 B per Gaussian (20 + 36 read, 16 + 16 written) over 8 TB/s;
  (iii) the opacity reset at 1M against the stock sequence.

Every fused call goes straight to the C entry point with buffers allocated beforehand, so that the kernels are what is timed; wall
time between two events on the stream, the candidates alternated call by call in a rotating order, medians.  The stock sweep is timed
--stock-sweep-steps times (it takes a good part of a second).  The measurement runs in two fresh processes one after the other; one
JSON line per process, printed and appended to profiles/filter3d_bench.jsonl.

    python tools/filter3d_bench.py --steps 30 --warmup 5
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

HBM_BYTES_PER_S = 8e12
ACT_BYTES = 88
# the sweep's inner loop per Gaussian-camera pair: 17 fma (three dot products as chains, four bounds, four differences), 2 mul,
# 5 mov (the translation and the principal point move from scalar to vector registers), 7 of the min / max / cmp / cndmask kind;
# wave-instructions per second of the whole chip per kind, each kind issued alone.  A mix issues faster than its kinds priced one by
# one (the probe's forward-blend mix: 740 - 880 G/s against 505 - 630 for its parts), so the floor is the loop's 31 instructions at
# the fastest rate the probe recorded for a mix; the per-kind price is given beside it.
SWEEP_LOOP = {"fma": (17, 630e9), "mul": (2, 852e9), "mov": (5, 900e9), "select": (7, 540e9)}
MIX_RATE = 880e9


def child(args):
    import torch

    import fused_filter3d as ff
    import torch_filter3d as ref
    from diff_gaussian_rasterization import _C
    if args.library:
        _C.use_library(os.path.abspath(args.library))
    dev = torch.device("cuda:0")
    lib = ff._lib()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def medians(runs, steps=None, warmup=None):
        steps, warmup = steps or args.steps, args.warmup if warmup is None else warmup
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

    out = {"steps": args.steps, "warmup": args.warmup, "library": os.path.basename(args.library) if args.library else None, "sweep": {},
           "activations": {}}
    C = args.cameras
    cams = ref.ring_cameras(C, W=1600, H=1064)
    for c in cams:   # on the device, as a training set's cameras are
        c.world_view_transform = c.world_view_transform.to(dev)
    rec = ff.pack_cameras(cams, dev)
    wave_s_per_pair = sum(n / rate for n, rate in SWEEP_LOOP.values())
    for P in (int(v) for v in args.sizes.split(",")):
        g = torch.Generator(device=dev).manual_seed(P % 1000)
        xyz = 6.0 * torch.rand(P, 3, device=dev, generator=g) - 3.0
        filt = torch.empty(P, 1, device=dev)
        scratch = torch.empty(lib.gsr_filter3d_scratch_bytes(P), dtype=torch.uint8, device=dev)

        def fused():
            check(lib.gsr_filter3d_compute(P, C, xyz.data_ptr(), rec.data_ptr(), 0, filt.data_ptr(), scratch.data_ptr(), stream))

        def stock():
            return stock_sweep(torch, xyz, cams)

        fused()
        s = stock()
        agree = float(((filt - s).abs() / s).median())
        differ = int(((filt - s).abs() > 1e-5 * s).sum())
        med = medians({"fused": fused})
        med.update(medians({"stock": stock}, steps=args.stock_sweep_steps, warmup=1))
        priced_ms = (P / 64.0) * C * wave_s_per_pair * 1e3
        floor_ms = (P / 64.0) * C * sum(n for n, _ in SWEEP_LOOP.values()) / MIX_RATE * 1e3
        out["sweep"][str(P)] = {"cameras": C, "i_fused_ms": round(med["fused"], 4), "i_stock_pytorch_ms": round(med["stock"], 2),
                                "i_stock_over_fused": round(med["stock"] / med["fused"], 1), "valu_floor_ms": round(floor_ms, 4),
                                "fused_over_floor": round(med["fused"] / floor_ms, 2), "priced_per_kind_ms": round(priced_ms, 4),
                                "median_rel_diff_to_stock_fp32": agree,
                                "rows_differing_from_stock_fp32": differ}

        opacity, scaling = 16.0 * torch.rand(P, 1, device=dev, generator=g) - 8.0, 11.0 * torch.rand(P, 3, device=dev, generator=g) - 9.0
        f3 = torch.exp(torch.rand(P, 1, device=dev, generator=g) * 6.9 - 9.2)
        g_o, g_s = torch.randn(P, 1, device=dev, generator=g), torch.randn(P, 3, device=dev, generator=g)
        o, sc, d_o, d_s = (torch.empty_like(t) for t in (opacity, scaling, opacity, scaling))

        def fused_act():
            check(lib.gsr_filter3d_activate(P, opacity.data_ptr(), scaling.data_ptr(), f3.data_ptr(), o.data_ptr(), sc.data_ptr(), stream))
            check(lib.gsr_filter3d_activate_backward(P, opacity.data_ptr(), scaling.data_ptr(), f3.data_ptr(), g_o.data_ptr(), g_s.data_ptr(),
                                                     d_o.data_ptr(), d_s.data_ptr(), stream))

        def stock_act():
            l, ls = opacity.detach().requires_grad_(True), scaling.detach().requires_grad_(True)
            so, ss = ref.stock_activations(l, ls, f3, torch.float32)
            torch.autograd.backward((so, ss), (g_o, g_s))
            return so.detach(), ss.detach(), l.grad, ls.grad

        fused_act()
        so, ss, sl, sls = stock_act()
        med = medians({"fused": fused_act, "stock": stock_act})
        floor_ms = P * ACT_BYTES / HBM_BYTES_PER_S * 1e3
        out["activations"][str(P)] = {"ii_fused_fwd_bwd_ms": round(med["fused"], 4), "ii_stock_pytorch_ms": round(med["stock"], 4),
                                      "ii_stock_over_fused": round(med["stock"] / med["fused"], 2), "streaming_floor_ms": round(floor_ms, 4),
                                      "fused_over_floor": round(med["fused"] / floor_ms, 2),
                                      "fused_bytes_per_s": round(P * ACT_BYTES / (med["fused"] * 1e-3), -9),
                                      "agreement_with_stock_fp32": {"opacities_rel_median": float(((o - so).abs() / so.abs().clamp(min=1e-30)).median()),
                                                                    "scales_rel_max": float(((sc - ss).abs() / ss).max()),
                                                                    "stock_nan_gradients": int(torch.isnan(sls).sum())}}

    P = args.reset_size
    g = torch.Generator(device=dev).manual_seed(3)
    base = 16.0 * torch.rand(P, 1, device=dev, generator=g) - 8.0
    scaling = 11.0 * torch.rand(P, 3, device=dev, generator=g) - 9.0
    f3 = torch.exp(torch.rand(P, 1, device=dev, generator=g) * 6.9 - 9.2)
    logits, m, v = base.clone(), torch.rand(P, 1, device=dev), torch.rand(P, 1, device=dev)
    s_logits, sm, sv = base.clone(), m.clone(), v.clone()

    def fused_reset():   # the logits are restored first on both sides: a reset of reset logits would change nothing
        logits.copy_(base)
        check(lib.gsr_filter3d_reset_opacity(P, logits.data_ptr(), scaling.data_ptr(), f3.data_ptr(), 0.01, m.data_ptr(), v.data_ptr(), stream))

    def stock_reset():
        s_logits.copy_(base)
        s_logits.copy_(ref.stock_reset_logits(s_logits, scaling, f3, 0.01, torch.float32))
        sm.zero_()
        sv.zero_()

    fused_reset()
    stock_reset()
    med = medians({"fused": fused_reset, "stock": stock_reset})
    out["reset"] = {"P": P, "iii_fused_ms": round(med["fused"], 4), "iii_stock_pytorch_ms": round(med["stock"], 4),
                    "iii_stock_over_fused": round(med["stock"] / med["fused"], 2),
                    "stock_nan_rows": int(torch.isnan(s_logits).sum()), "max_abs_diff_where_stock_is_finite":
                    float((logits - s_logits)[torch.isfinite(s_logits)].abs().max())}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


def stock_sweep(torch, xyz, cams):
    """Mip-Splatting's compute_3D_filter as published, fp32 on the device of xyz"""
    import math
    distance = torch.ones(xyz.shape[0], device=xyz.device) * 100000.0
    valid_points = torch.zeros(xyz.shape[0], device=xyz.device, dtype=torch.bool)
    focal_length = 0.0
    for cam in cams:
        W, H = cam.image_width, cam.image_height
        fx, fy = W / (2.0 * math.tan(0.5 * cam.FoVx)), H / (2.0 * math.tan(0.5 * cam.FoVy))
        wvt = cam.world_view_transform
        xyz_cam = xyz @ wvt[:3, :3] + wvt[3, :3][None, :]
        z = xyz_cam[:, 2]
        in_front = z > 0.2
        u = xyz_cam[:, 0] / torch.clamp(z, min=0.001) * fx + W / 2.0
        v = xyz_cam[:, 1] / torch.clamp(z, min=0.001) * fy + H / 2.0
        in_screen = torch.logical_and(torch.logical_and(u >= -0.15 * W, u <= W * 1.15), torch.logical_and(v >= -0.15 * H, v <= 1.15 * H))
        valid = torch.logical_and(in_front, in_screen)
        distance[valid] = torch.min(distance[valid], z[valid])
        valid_points = torch.logical_or(valid_points, valid)
        focal_length = max(focal_length, fx)
    distance[~valid_points] = distance[valid_points].max()
    return (distance / focal_length * (0.2 ** 0.5))[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1000000,6000000")
    ap.add_argument("--cameras", type=int, default=200)
    ap.add_argument("--stock-sweep-steps", type=int, default=3)
    ap.add_argument("--reset-size", type=int, default=1000000)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--library", default=None, help="a variant build of libgsr_hip.so (csrc/Makefile, `make variant`) to run instead")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "filter3d_bench.jsonl"))
    ap.add_argument("--child", action="store_true", help="measure in this process (what the tool starts --processes times)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    for _ in range(args.processes):   # fresh processes, one after the other; this one never opens the device
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"], check=True)


if __name__ == "__main__":
    main()
