"""The fused MLP (fused_mlp.mlp) against the stock float32 nn.Sequential with autograd, on the same GPU in the same process.

    python tools/mlp_bench.py [--rows 1000000 6000000] [--runs 30] [--warmup 5] [--out profiles/mlp_bench.jsonl]

Buffers are allocated beforehand; a run's wall time is taken between two events; the two candidates alternate run by run; the
figure is the median of --runs runs after --warmup.  One JSON line per shape, row count and pass (forward, forward + backward) with
  fused_ms, stock_ms          the two medians
  floor_bytes_ms              the bytes that must move (x and y forward; x, dy and dx more backward) over 8 TB/s
  floor_flops_ms              the issued flops over the fp32-MFMA peak of 157 TF: 2 N sum d_l d_{l-1} forward, four times that with the
                              recompute, dx and dW
  fused_peak_mb, stock_peak_mb   peak memory during one forward + backward above the inputs (x, dy, the parameters) and the
                              outputs (y and the gradients the step leaves behind)
  stock_dw_changes            whether the stock dW of the first layer differs between two runs; fused_dw_changes likewise
Run it in two fresh processes and keep both lines."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401
import fused_mlp  # noqa: E402

SHAPES = {
    "scaffold_35_32_70_tanh": dict(in_dim=35, out_dim=70, hidden=32, hidden_layers=1, output_activation="tanh"),
    "w64_h2": dict(in_dim=64, out_dim=3, hidden=64, hidden_layers=2),
    "w64_h4": dict(in_dim=64, out_dim=3, hidden=64, hidden_layers=4),
    "enc_d4_l10_64_64_3": dict(in_dim=4, out_dim=3, hidden=64, hidden_layers=2, frequencies=10),
}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak_above(fn, y_bytes):
    """Peak allocation during fn() above what was allocated before it, less y and what fn() leaves allocated (the gradients), in MB"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    left = torch.cuda.memory_allocated() - base
    return (torch.cuda.max_memory_allocated() - base - left - y_bytes) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000000, 6000000])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = []
    for name in args.shapes:
        kw = SHAPES[name]
        m = fused_mlp.TinyMLP(**kw).to(dev)
        seq = m.to_sequential()
        widths = [m.weights[0].shape[1]] + [w.shape[0] for w in m.weights]
        mac = sum(a * b for a, b in zip(widths[:-1], widths[1:]))
        for N in args.rows:
            x = (torch.randn(N, kw["in_dim"], device=dev) * (0.01 if kw.get("frequencies") else 1.0)).requires_grad_(True)
            g = torch.randn(N, kw["out_dim"], device=dev)

            def fwd(net):
                with torch.no_grad():
                    return net(x)

            def fwd_bwd(net):
                x.grad = None
                for p in net.parameters():
                    p.grad = None
                net(x).backward(g)

            for label, step in (("forward", fwd), ("forward_backward", fwd_bwd)):
                t = {"fused": [], "stock": []}
                for it in range(args.warmup + args.runs):
                    for who, net in (("fused", m), ("stock", seq)):   # the candidates alternate
                        ms = timed(lambda: step(net))
                        if it >= args.warmup:
                            t[who].append(ms)
                bwd = label != "forward"
                nbytes = 4 * N * (kw["in_dim"] + kw["out_dim"]) * (2 if bwd else 1) + (4 * N * kw["in_dim"] if bwd else 0)
                rec = dict(shape=name, widths=widths, rows=N, what=label, fused_ms=round(statistics.median(t["fused"]), 4),
                           stock_ms=round(statistics.median(t["stock"]), 4), floor_bytes_ms=round(nbytes / 8e12 * 1e3, 4),
                           floor_flops_ms=round(2 * N * mac * (4 if bwd else 1) / 157e12 * 1e3, 4), runs=args.runs, pid=os.getpid())
                if bwd:
                    for net in (m, seq):   # no gradient from an earlier step is freed inside the measured one
                        x.grad = None
                        for q in net.parameters():
                            q.grad = None
                    rec["fused_peak_mb"] = round(peak_above(lambda: fwd_bwd(m), 4 * N * kw["out_dim"]), 1)
                    x.grad = None
                    rec["stock_peak_mb"] = round(peak_above(lambda: fwd_bwd(seq), 4 * N * kw["out_dim"]), 1)
                    changes = {}
                    for who, net, first in (("fused", m, m.weights[0]), ("stock", seq, [q for q in seq if isinstance(q, torch.nn.Linear)][0].weight)):
                        fwd_bwd(net)
                        one = first.grad.clone()
                        fwd_bwd(net)
                        changes[who] = not torch.equal(one, first.grad)
                    rec["fused_dw_changes"], rec["stock_dw_changes"] = changes["fused"], changes["stock"]
                rec["speedup"] = round(rec["stock_ms"] / rec["fused_ms"], 3)
                lines.append(rec)
                print(json.dumps(rec), flush=True)
            del x, g
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
