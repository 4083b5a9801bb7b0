"""Cost and memory of the fused densification (include/gsr_densify.h, fused_densify.py) against the stock-PyTorch sequence a user of the
reference writes (GaussianModel.densify_and_prune: clone, then split, then prune, each a round of boolean-mask indexing and torch.cat
over six parameter tensors and their twelve moment tensors), on the same GPU in the same process.

  sizes   1M and 6M Gaussians at SH degree 3 (59 words per row), with moments; 10 % of the rows cloned, 10 % split, 5 % pruned
  fused   gsr_densify_plan, the read-back of the four totals, gsr_densify_apply: straight at the C entry points, every buffer and
          every output allocated beforehand
  stock   the cat and mask sequence with the same three row sets and the same noise; torch.cuda.empty_cache(), which the reference
          calls at the end, is left out.  The random draw is left out on both sides
  time    wall time between two events on the stream, the two alternated call by call in a rotating order, medians
  memory  torch.cuda.max_memory_allocated over one call minus what was allocated before it (the model's own bytes), the fused side
          through fused_densify.densify, which allocates its outputs, scratch and map
  floor   the bytes that must move over 8 TB/s: every input word read once, every output word written once, the map written and read

The measurement runs in two fresh processes one after the other; one JSON line per process, printed and appended to
profiles/densify_bench.jsonl.

    python tools/densify_bench.py --steps 30 --warmup 5
"""
import argparse
import ctypes
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
KEEP, PRUNE, CLONE, SPLIT = 0, 1, 2, 3


def stock_densify_and_prune(params, moments, clone, split, prune, noise):
    """the reference's sequence after its masks are known -> (params, moments)"""
    import torch

    import torch_mcmc
    params, moments = list(params), list(moments)
    P = params[0].shape[0]

    def append(new):
        for k, t in enumerate(new):
            params[k] = torch.cat((params[k], t), dim=0)
            moments[k] = tuple(torch.cat((s, torch.zeros_like(t)), dim=0) for s in moments[k])

    def keep(mask):
        for k in range(len(params)):
            params[k] = params[k][mask]
            moments[k] = tuple(s[mask] for s in moments[k])

    def padded(mask):
        return torch.cat((mask, torch.zeros(params[0].shape[0] - mask.shape[0], dtype=torch.bool, device=mask.device)))

    append([t[clone] for t in params])
    sel = padded(split)
    new = [t[sel].repeat(*([2] + [1] * (t.dim() - 1))) for t in params]
    stds = torch.exp(params[4][sel]).repeat(2, 1)
    q = params[5][sel]
    rots = torch_mcmc.rotation_matrices(q / q.norm(dim=-1, keepdim=True)).repeat(2, 1, 1)
    new[0] = torch.bmm(rots, (stds * noise).unsqueeze(-1)).squeeze(-1) + params[0][sel].repeat(2, 1)
    new[4] = torch.log(stds / (0.8 * 2))
    append(new)
    keep(~padded(sel))
    keep(~padded(prune[~split]))
    assert params[0].shape[0] == P + int(clone.sum()) + int(split.sum()) - int(prune.sum())
    return params, moments


def child(args):
    import torch

    import fused_densify as fd
    from diff_gaussian_rasterization import _C
    if args.library:
        _C.use_library(os.path.abspath(args.library))
    dev = torch.device("cuda:0")
    lib = fd._lib()
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

    out = {"steps": args.steps, "warmup": args.warmup, "library": os.path.basename(args.library) if args.library else None, "sizes": {}}
    for P in (int(v) for v in args.sizes.split(",")):
        g = torch.Generator(device=dev).manual_seed(P % 1000)
        rand = lambda *s: torch.rand(*s, device=dev, generator=g)
        params = [3 * torch.randn(P, 3, device=dev, generator=g), torch.randn(P, 1, 3, device=dev, generator=g),
                  torch.randn(P, 15, 3, device=dev, generator=g), 18 * rand(P, 1) - 9, 8 * rand(P, 3) - 6,
                  torch.randn(P, 4, device=dev, generator=g) * (0.1 + 9.9 * rand(P, 1))]
        moments = [(torch.randn(p.shape, device=dev, generator=g), torch.rand(p.shape, device=dev, generator=g)) for p in params]
        u = rand(P)
        action = torch.where(u < 0.10, CLONE, torch.where(u < 0.20, SPLIT, torch.where(u < 0.25, PRUNE, KEEP))).to(torch.uint8)
        clone, split, prune = action == CLONE, action == SPLIT, action == PRUNE
        K, C, S = int(((action == KEEP) | clone).sum()), int(clone.sum()), int(split.sum())
        Pout = K + C + 2 * S
        noise = torch.randn(2 * S, 3, device=dev, generator=g)
        words = sum(p.numel() // P for p in params)

        # memory, one call each, before anything of the timed runs is allocated
        rows = [(p, m, v) for p, (m, v) in zip(params, moments)]
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        fused_out, _, counts = fd.densify(rows, action, noise=noise)
        torch.cuda.synchronize(dev)
        fused_peak = torch.cuda.max_memory_allocated(dev) - base
        assert counts == (K, C, S)
        torch.cuda.reset_peak_memory_stats(dev)
        base_stock = torch.cuda.memory_allocated(dev)
        stock_params, stock_moments = stock_densify_and_prune(params, moments, clone, split, prune, noise)
        torch.cuda.synchronize(dev)
        stock_peak = torch.cuda.max_memory_allocated(dev) - base_stock
        first = K + C
        agree = {"rows_equal": all(bool(torch.equal(a[0], b)) for k, (a, b) in enumerate(zip(fused_out, stock_params)) if k not in (0, 4)),
                 "survivors_and_clones_equal": bool(torch.equal(fused_out[0][0][:first], stock_params[0][:first]) and torch.equal(fused_out[4][0][:first], stock_params[4][:first])),
                 "moments_equal": all(bool(torch.equal(a[1], b[0]) and torch.equal(a[2], b[1])) for a, b in zip(fused_out, stock_moments)),
                 "children_xyz_max_abs": float((fused_out[0][0][first:] - stock_params[0][first:]).abs().max()),
                 "children_log_scale_max_abs": float((fused_out[4][0][first:] - stock_params[4][first:]).abs().max())}
        del stock_params, stock_moments

        # time: the fused side straight at the C entry points, writing into the outputs of the call above
        scratch = torch.empty(lib.gsr_densify_scratch_bytes(P), dtype=torch.uint8, device=dev)
        totals = torch.empty(4, dtype=torch.int32, device=dev)
        src_of = torch.empty(Pout, dtype=torch.int32, device=dev)
        table = (fd.DensifyGroup * 6)(*[fd.DensifyGroup(p.data_ptr(), m.data_ptr(), v.data_ptr(), op.data_ptr(), om.data_ptr(), ov.data_ptr(), p.numel() // P, 0)
                                        for (p, m, v), (op, om, ov) in zip(rows, fused_out)])

        def fused():
            check(lib.gsr_densify_plan(P, action.data_ptr(), scratch.data_ptr(), totals.data_ptr(), stream))
            k, c, s, bad = totals.tolist()
            a = fd.DensifyArgs(P=P, K=k, C=c, S=s, ngroups=6, xyz_group=0, scale_group=4, rotation_group=5, groups=table, action=action.data_ptr(),
                               scratch=scratch.data_ptr(), noise=noise.data_ptr(), src_of=src_of.data_ptr(), stream=stream)
            check(lib.gsr_densify_apply(ctypes.byref(a)))

        a_fixed = fd.DensifyArgs(P=P, K=K, C=C, S=S, ngroups=6, xyz_group=0, scale_group=4, rotation_group=5, groups=table, action=action.data_ptr(),
                                 scratch=scratch.data_ptr(), noise=noise.data_ptr(), src_of=src_of.data_ptr(), stream=stream)
        med = medians({"fused": fused, "stock": lambda: stock_densify_and_prune(params, moments, clone, split, prune, noise),
                       "plan": lambda: check(lib.gsr_densify_plan(P, action.data_ptr(), scratch.data_ptr(), totals.data_ptr(), stream)),
                       "apply": lambda: check(lib.gsr_densify_apply(ctypes.byref(a_fixed)))})
        floor_bytes = 3 * 4 * words * (P + Pout) + 8 * Pout + P
        floor_ms = floor_bytes / HBM_BYTES_PER_S * 1e3
        out["sizes"][str(P)] = {"P": P, "K": K, "C": C, "S": S, "P_out": Pout, "sh_degree": 3, "words_per_row": words,
                                "fused_ms": round(med["fused"], 4), "plan_ms": round(med["plan"], 4), "apply_ms": round(med["apply"], 4),
                                "stock_pytorch_ms": round(med["stock"], 3), "stock_over_fused": round(med["stock"] / med["fused"], 2),
                                "floor_ms": round(floor_ms, 4), "fused_over_floor": round(med["fused"] / floor_ms, 2),
                                "apply_over_floor": round(med["apply"] / floor_ms, 2), "apply_bytes_per_s": round(floor_bytes / (med["apply"] * 1e-3), -9),
                                "model_bytes": base, "fused_peak_bytes_above_model": fused_peak, "stock_peak_bytes_above_model": stock_peak,
                                "output_bytes": 3 * 4 * words * Pout, "agreement_with_stock": agree}
        del params, moments, rows, fused_out, table, scratch, src_of, noise, action
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
    ap.add_argument("--out", default=os.path.join(R, "profiles", "densify_bench.jsonl"))
    ap.add_argument("--child", action="store_true", help="measure in this process (what the tool starts --processes times)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    for _ in range(args.processes):   # fresh processes, one after the other; this one never opens the device
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"], check=True)


if __name__ == "__main__":
    main()
