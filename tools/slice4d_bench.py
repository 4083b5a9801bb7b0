"""Cost of the fused 4D time slice and harmonic colour coefficients (include/gsr_slice4d.h, fused_slice4d.py) against the
stock-PyTorch float32 sequences a user writes, on the same GPU in the same process, at 1M and 6M Gaussians:

  (i)   slice_at forward plus backward against tests/torch_slice4d.slice4d() in float32 with autograd (two 4 x 4 matrix builds, two
        bmm, slicing, a division, exp, sigmoid, and as many launches again backward) and against the streaming floor of 284 B per
        Gaussian: 68 read and 40 written forward; 68 + 40 read (the incoming gradients of means3D, cov3D and opacities) and 68 written
        backward;
  (ii)  harmonic_features forward plus backward at N = 2, M = 16 against the stock sequence (cos, a broadcast product, a sum) with
        autograd and against the streaming floor of 1932 B per Gaussian: 580 read and 192 written forward; 388 + 192 read (harmonic 0
        is not needed for dL/dt) and 580 written backward.

Every fused call goes straight to the C entry point with buffers allocated beforehand, so that the kernels are what is timed; wall
time between two events on the stream, the candidates alternated call by call in a rotating order, medians.  The measurement runs in
two fresh processes one after the other; one JSON line per process, printed and appended to profiles/slice4d_bench.jsonl.

    python tools/slice4d_bench.py --steps 30 --warmup 5
"""
import argparse
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
SLICE_BYTES = {"fwd": 68 + 40, "bwd": 68 + 40 + 68}
N, M = 2, 16
HARM_BYTES = {"fwd": (N + 1) * M * 12 + 4 + M * 12, "bwd": N * M * 12 + 4 + M * 12 + (N + 1) * M * 12 + 4}


def child(args):
    import torch

    import fused_slice4d as fs
    import torch_slice4d as ref
    from diff_gaussian_rasterization import _C
    if args.library:
        _C.use_library(os.path.abspath(args.library))
    dev = torch.device("cuda:0")
    lib = fs._lib()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def medians(runs):
        ms = {k: [] for k in runs}
        names = list(runs)
        for it in range(args.warmup + args.steps):
            for k in names[it % len(names):] + names[:it % len(names)]:   # rotated: no candidate always runs behind the same one
                t = timed(runs[k])
                if it >= args.warmup:
                    ms[k].append(t)
        return {k: statistics.median(v) for k, v in ms.items()}

    def check(rc):
        assert rc == 0, lib.gsr_last_error()

    def row(med, nbytes, P):
        floor = {k: P * b / HBM_BYTES_PER_S * 1e3 for k, b in nbytes.items()}
        fused = med["fwd"] + med["bwd"]
        return {"fused_fwd_ms": round(med["fwd"], 4), "fused_bwd_ms": round(med["bwd"], 4), "fused_fwd_bwd_ms": round(fused, 4),
                "stock_pytorch_fp32_fwd_bwd_ms": round(med["stock"], 3), "stock_over_fused": round(med["stock"] / fused, 1),
                "streaming_floor_fwd_ms": round(floor["fwd"], 4), "streaming_floor_bwd_ms": round(floor["bwd"], 4),
                "fwd_over_floor": round(med["fwd"] / floor["fwd"], 2), "bwd_over_floor": round(med["bwd"] / floor["bwd"], 2),
                "fwd_bytes_per_s": round(P * nbytes["fwd"] / (med["fwd"] * 1e-3), -9), "bwd_bytes_per_s": round(P * nbytes["bwd"] / (med["bwd"] * 1e-3), -9)}

    out = {"steps": args.steps, "warmup": args.warmup, "library": os.path.basename(args.library) if args.library else None, "slice": {},
           "harmonic": {"N": N, "M": M}}
    time, period = 0.5, 0.8
    for P in (int(v) for v in args.sizes.split(",")):
        g = torch.Generator(device=dev).manual_seed(P % 1000)
        n = lambda *s: torch.randn(*s, device=dev, generator=g)
        leaves = [n(P, 3), time - 0.3 * n(P, 1), -2.0 + 0.7 * n(P, 3), -2.0 + 0.7 * n(P, 1), n(P, 4), n(P, 4), 2.0 * n(P, 1)]
        gin = [n(P, 3), n(P, 6), n(P, 1)]
        outs = [torch.empty(P, c, device=dev) for c in (3, 6, 1)]
        grads = [torch.empty_like(x) for x in leaves]
        lp, gp, op, dp = ([t.data_ptr() for t in ts] for ts in (leaves, gin, outs, grads))

        def fwd():
            check(lib.gsr_slice4d_forward(P, *lp, time, 1.0, 0.05, *op, None, stream))

        def bwd():
            check(lib.gsr_slice4d_backward(P, *lp, time, 1.0, 0.05, *gp, None, *dp, stream))

        def stock():
            x = {k: t.detach().requires_grad_(True) for k, t in zip(ref.LEAVES, leaves)}
            sl = ref.slice4d(x, time, dtype=torch.float32)
            torch.autograd.backward((sl.means3D, sl.cov3D, sl.opacities), gin)
            return sl

        fwd()
        bwd()
        sl = stock()
        live = ~sl.mask
        rel = ((outs[1] - sl.cov3D.detach()).abs() / outs[1].abs().clamp(min=1e-30))[live]
        agree = {"cov3D_rel_median": float(rel.median()), "cov3D_rel_max": float(rel.max()),
                 "masks_differ": int(((outs[2][:, 0] == 0) != sl.mask).sum())}
        del sl
        out["slice"][str(P)] = dict(row(medians({"fwd": fwd, "bwd": bwd, "stock": stock}), SLICE_BYTES, P), agreement_with_stock_fp32=agree)

        f, shs_g = n(P, N + 1, M, 3), n(P, M, 3)
        t = leaves[1]
        shs, d_f, d_t = torch.empty(P, M, 3, device=dev), torch.empty_like(f), torch.empty_like(t)
        k = (2.0 * math.pi / period) * torch.arange(N + 1, device=dev, dtype=torch.float32)[None, :]

        def hfwd():
            check(lib.gsr_harmonic_features(P, N, M, f.data_ptr(), t.data_ptr(), time, period, shs.data_ptr(), stream))

        def hbwd():
            check(lib.gsr_harmonic_features_backward(P, N, M, f.data_ptr(), t.data_ptr(), time, period, shs_g.data_ptr(), d_f.data_ptr(), d_t.data_ptr(),
                                                     stream))

        def hstock():
            a, b = f.detach().requires_grad_(True), t.detach().requires_grad_(True)
            s = (torch.cos(k * (time - b))[:, :, None, None] * a).sum(1)
            s.backward(shs_g)
            return s.detach()

        hfwd()
        hbwd()
        s = hstock()
        agree = float((shs - s).abs().max())
        del s
        out["harmonic"][str(P)] = dict(row(medians({"fwd": hfwd, "bwd": hbwd, "stock": hstock}), HARM_BYTES, P), max_abs_diff_to_stock_fp32=agree)
        del leaves, gin, outs, grads, f, shs_g, shs, d_f, d_t
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1000000,6000000")
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--library", default=None, help="a variant build of libgsr_hip.so (csrc/Makefile, `make variant`) to run instead")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "slice4d_bench.jsonl"))
    ap.add_argument("--child", action="store_true", help="measure in this process (what the tool starts --processes times)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    for _ in range(args.processes):   # fresh processes, one after the other; this one never opens the device
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"], check=True)


if __name__ == "__main__":
    main()
