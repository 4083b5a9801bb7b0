"""Cost of the fused MCMC pieces (include/gsr_mcmc.h, fused_mcmc.py) against the stock-PyTorch fp32 sequences a user writes, on the
same GPU in the same process:

  (i)   noise injection at 1M and 6M Gaussians against gsplat's inject_noise_to_position in stock PyTorch (normalise, R, R S, a bmm, a
        sigmoid, the gate, an einsum, an add; the randn left out on both sides) and against the streaming floor of 68 B per Gaussian
        (56 read, 12 written) over 8 TB/s;
  (ii)  relocation at 1M Gaussians with 5 % dead rows and SH degree 3 (six parameter tensors, twelve moment tensors) against the
        stock indexing sequence: a bincount, the binomial sum as a table product, logit and log, index_put on six tensors and on
        twelve moments.  The draw of the sources is left out on both sides;
  (iii) the regulariser with its backward at 1M Gaussians against the stock expression with autograd.

Every fused call goes straight to the C entry point with buffers allocated beforehand, so that the kernels are what is timed; wall
time between two events on the stream, the candidates alternated call by call in a rotating order, medians.  The measurement runs
in two fresh processes one after the other; one JSON line per process, printed and appended to profiles/mcmc_bench.jsonl.

    python tools/mcmc_bench.py --steps 30 --warmup 5
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
NOISE_BYTES = 68


def stock_relocate(params, moments, dst, src, table, min_opacity=0.005):
    """gsplat's relocate after the draw, with compute_relocation as a (51, 51) table product in place of its compiled kernel"""
    import torch
    P = params[3].shape[0]
    opac = torch.sigmoid(params[3]).flatten()
    ratios = (torch.bincount(src, minlength=P)[src] + 1).clamp(min=1, max=51)
    o = opac[src].double()
    new_o = 1.0 - (1.0 - o) ** (1.0 / ratios.double())
    powers = new_o[:, None] ** torch.arange(1, 52, device=o.device, dtype=torch.float64)[None]
    denom = (table[ratios - 1] * powers).sum(1)
    new_scales = (o / denom)[:, None] * torch.exp(params[4][src]).double()
    params[3][src] = torch.logit(new_o.clamp(min_opacity, 1.0 - 2.0 ** -23)).float()[:, None]
    params[4][src] = torch.log(new_scales).float()
    for p in params:
        p[dst] = p[src]
    for m, v in moments:
        m[src] = 0
        v[src] = 0


def child(args):
    import torch

    import fused_mcmc as fm
    import torch_mcmc as ref
    from diff_gaussian_rasterization import _C
    if args.library:
        _C.use_library(os.path.abspath(args.library))
    dev = torch.device("cuda:0")
    lib = fm._lib()
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

    def leaves(P, rest):
        g = torch.Generator(device=dev).manual_seed(P % 1000 + rest)
        rand = lambda *s: torch.rand(*s, device=dev, generator=g)
        return [3 * torch.randn(P, 3, device=dev, generator=g), torch.randn(P, 1, 3, device=dev, generator=g),
                torch.randn(P, rest, 3, device=dev, generator=g), 18 * rand(P, 1) - 9, 8 * rand(P, 3) - 6,
                torch.randn(P, 4, device=dev, generator=g) * (0.1 + 9.9 * rand(P, 1))]

    out = {"steps": args.steps, "warmup": args.warmup, "library": os.path.basename(args.library) if args.library else None, "noise": {}}
    scaler = 0.8
    for P in (int(v) for v in args.noise_sizes.split(",")):
        xyz, _, _, opacity, scaling, rotation = leaves(P, 0)
        eps = torch.randn(P, 3, device=dev)
        xs = xyz.clone()

        def fused():
            check(lib.gsr_mcmc_noise(P, xyz.data_ptr(), opacity.data_ptr(), scaling.data_ptr(), rotation.data_ptr(), eps.data_ptr(), scaler, stream))

        def stock():
            xs.add_(ref.stock_noise_displacement(opacity, scaling, rotation, eps, scaler))

        zero = torch.zeros_like(xyz)
        d = fm.inject_noise(zero, opacity, scaling, rotation, scaler, noise=eps)
        s = ref.stock_noise_displacement(opacity, scaling, rotation, eps, scaler)
        med = medians({"fused": fused, "stock": stock})
        floor_ms = P * NOISE_BYTES / HBM_BYTES_PER_S * 1e3
        out["noise"][str(P)] = {"i_fused_ms": round(med["fused"], 4), "i_stock_pytorch_ms": round(med["stock"], 4),
                                "i_stock_over_fused": round(med["stock"] / med["fused"], 2), "streaming_floor_ms": round(floor_ms, 4),
                                "fused_over_floor": round(med["fused"] / floor_ms, 2), "fused_bytes_per_s": round(P * NOISE_BYTES / (med["fused"] * 1e-3), -9),
                                "agreement_with_stock_fp32": float((d - s).norm(dim=1).max() / s.norm(dim=1).max())}

    P, rest = args.relocate_size, 15
    params = leaves(P, rest)
    params[3].clamp_(min=-2.9)
    D = P // 20
    g = torch.Generator(device=dev).manual_seed(9)
    dst = torch.randperm(P, device=dev, generator=g)[:D]
    params[3][dst] = -7.0
    opac = torch.sigmoid(params[3]).flatten()
    src = torch.multinomial(torch.where(opac <= 0.005, torch.zeros_like(opac), opac), D, replacement=True, generator=g)
    moments = [(torch.randn_like(p), torch.rand_like(p)) for p in params]
    fused_params, fused_moments = [p.clone() for p in params], [(m.clone(), v.clone()) for m, v in moments]
    table = torch.tensor([[math.comb(n, k + 1) * (-1) ** k / math.sqrt(k + 1) if k < n else 0.0 for k in range(51)] for n in range(1, 52)],
                         dtype=torch.float64, device=dev)
    groups = (fm.McmcGroup * 6)(*[fm.McmcGroup(p.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel() // P) for p, (m, v) in zip(fused_params, fused_moments)])
    counts = torch.empty(P, dtype=torch.int32, device=dev)
    a = fm.RelocateArgs(P=P, D=D, ngroups=6, opacity_group=3, scale_group=4, zero_src_moments=1, min_opacity=0.005, groups=groups,
                        dst=dst.data_ptr(), src=src.data_ptr(), counts=counts.data_ptr(), stream=stream)

    def fused_relocate():
        check(lib.gsr_mcmc_relocate(ctypes.byref(a)))

    # the first call of each on the same state: the two compute the same thing
    fused_relocate()
    stock_relocate(params, moments, dst, src, table)
    agree = {"logit": float((fused_params[3] - params[3]).abs().max()), "log_scale": float((fused_params[4] - params[4]).abs().max()),
             "rows_equal": all(bool(torch.equal(x, y)) for k, (x, y) in enumerate(zip(fused_params, params)) if k not in (3, 4)),
             "moments_equal": all(bool(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])) for x, y in zip(fused_moments, moments))}
    med = medians({"fused": fused_relocate, "stock": lambda: stock_relocate(params, moments, dst, src, table)})
    row_floats = sum(p.numel() // P for p in params)
    floor_ms = D * (2 * row_floats + 2 * row_floats) * 4 / HBM_BYTES_PER_S * 1e3   # rows read and written, two moments written
    out["relocate"] = {"P": P, "D": D, "sh_degree": 3, "ii_fused_ms": round(med["fused"], 4), "ii_stock_pytorch_ms": round(med["stock"], 4),
                       "ii_stock_over_fused": round(med["stock"] / med["fused"], 2), "bytes_moved_floor_ms": round(floor_ms, 5),
                       "agreement_with_stock": agree}

    P = args.reg_size
    _, _, _, opacity, scaling, _ = leaves(P, 0)
    val, d_o, d_s = torch.empty(1, device=dev), torch.empty_like(opacity), torch.empty_like(scaling)
    scratch = torch.empty(lib.gsr_mcmc_regularizer_scratch_bytes(P), dtype=torch.uint8, device=dev)

    def fused_reg():
        check(lib.gsr_mcmc_regularizer(P, opacity.data_ptr(), scaling.data_ptr(), 0.01, 0.01, val.data_ptr(), d_o.data_ptr(), d_s.data_ptr(),
                                       scratch.data_ptr(), stream))

    def stock_reg():
        l, s = opacity.detach().requires_grad_(True), scaling.detach().requires_grad_(True)
        loss = 0.01 * torch.sigmoid(l).mean() + 0.01 * torch.exp(s).mean()
        loss.backward()
        return loss.detach(), l.grad, s.grad

    fused_reg()
    sv, sl, ss = stock_reg()
    med = medians({"fused": fused_reg, "stock": stock_reg})
    floor_ms = 2 * 16 * P / HBM_BYTES_PER_S * 1e3
    out["regularizer"] = {"P": P, "iii_fused_ms": round(med["fused"], 4), "iii_stock_pytorch_ms": round(med["stock"], 4),
                          "iii_stock_over_fused": round(med["stock"] / med["fused"], 2), "streaming_floor_ms": round(floor_ms, 4),
                          "fused_over_floor": round(med["fused"] / floor_ms, 2),
                          "agreement_with_stock_fp32": {"value_rel": abs(float(val) - float(sv)) / float(sv),
                                                        "d_opacity_rel": float(((d_o - sl).abs() / sl.abs().clamp(min=1e-30)).max()),
                                                        "d_scaling_rel": float(((d_s - ss).abs() / ss.abs()).max())}}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--noise-sizes", default="1000000,6000000")
    ap.add_argument("--relocate-size", type=int, default=1000000)
    ap.add_argument("--reg-size", type=int, default=1000000)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--library", default=None, help="a variant build of libgsr_hip.so (csrc/Makefile, `make variant`) to run instead")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "mcmc_bench.jsonl"))
    ap.add_argument("--child", action="store_true", help="measure in this process (what the tool starts --processes times)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    for _ in range(args.processes):   # fresh processes, one after the other; this one never opens the device
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"], check=True)


if __name__ == "__main__":
    main()
