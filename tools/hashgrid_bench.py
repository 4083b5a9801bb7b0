"""The fused hash-grid encoding (fused_hashgrid.hash_grid) against the stock float32 torch version with autograd (gathers that
materialise N x 2^D x F floats per level, and an index_add_ backward with float atomics), on the same GPU in the same process.

    python tools/hashgrid_bench.py [--shapes default ...] [--rows 1000000] [--runs 30] [--warmup 5] [--out profiles/hashgrid_bench.jsonl]

Buffers are allocated beforehand; a run's wall time is taken between two events; the two candidates alternate run by run; the
figure is the median of --runs runs after --warmup.  One JSON line per shape, row count and pass (forward; forward + backward with and
without dx) with
  fused_ms, stock_ms, speedup      the two medians and stock / fused
  floor_bytes_ms                   the bytes that must stream (x, y; backward: x again, dy, dtable, the scratch sums written by the
                                   clear and read by the convert, dx) over 8 TB/s
  floor_atomic_ms                  backward: the added bytes, N L 2^D F 8, over 1.3 TB/s, the rate measured for well-shaped float atomics
  fused_peak_mb, stock_peak_mb     peak memory during one forward + backward above the inputs and the outputs
  stock_dtable_changes, fused_dtable_changes   whether dtable differs between two runs
and, once per shape and row count (what = "table_backward"), the raw table backward alone:
  lds_levels, direct_levels        how many levels take which path
  table_ms, table_lds_ms           the backward for dtable alone over all levels, and over the LDS-path levels alone (a grid of those
                                   levels only); the direct levels are the difference
  added_tb_per_s                   N (direct levels) 2^D F 8 bytes over that difference: the rate of scattered 8-byte integer adds
  dx_ms                            the row-owner dx kernel alone
Run it in two fresh processes and keep both lines."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__  # noqa: E402,F401
import fused_hashgrid as fh  # noqa: E402
import torch_hashgrid as th  # noqa: E402

# (D, L, F, log2_hashmap_size, base_resolution, per_level_scale), default rows
SHAPES = {
    "default_d3_l16_f2_t19": ((3, 16, 2, 19, 16, 2.0), [1000000, 6000000]),                      # tiny-cuda-nn's defaults
    "compact3dgs_d3_l16_f2_t19_to4096": ((3, 16, 2, 19, 16, 1.4472692012786865), [1000000]),    # finest resolution 4096
    "d2_l16_f2_t19": ((2, 16, 2, 19, 16, 1.5), [1000000]),
    "d4_l16_f2_t19": ((4, 16, 2, 19, 8, 1.38), [1000000]),
}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, runs, warmup):
    t = [timed(fn) for _ in range(warmup + runs)]
    return statistics.median(t[warmup:])


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
    ap.add_argument("--rows", type=int, nargs="+", default=None)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hashgrid_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for name in args.shapes:
        cfg, rows = SHAPES[name]
        D, L, F, T, base, pls = cfg
        off, res, hashed, total = fh.level_layout(D, L, F, T, base, pls)
        paths = fh.level_paths(D, L, F, T, base, pls)
        nlds = sum(p == fh.PATH_LDS for p in paths)
        kw = dict(levels=L, features=F, log2_hashmap_size=T, base_resolution=base, per_level_scale=pls)
        table = (torch.rand((total, F), device=dev) * 2e-4 - 1e-4).requires_grad_(True)
        for N in args.rows or rows:
            x = torch.rand((N, D), device=dev)
            xg = x.clone().requires_grad_(True)
            g = torch.randn((N, L * F), device=dev)
            fused = lambda xx: fh.hash_grid(xx, table, **kw)
            stock = lambda xx: th.hash_grid_torch(xx, table, cfg)

            def fwd(net, xx):
                with torch.no_grad():
                    return net(xx)

            def fwd_bwd(net, xx):
                xx.grad = None
                table.grad = None
                net(xx).backward(g)

            common = dict(shape=name, cfg=list(cfg), rows=N, entries=total, runs=args.runs, pid=os.getpid())
            for label, step, xx in (("forward", fwd, x), ("forward_backward_dx", fwd_bwd, xg), ("forward_backward", fwd_bwd, x)):
                t = {"fused": [], "stock": []}
                for it in range(args.warmup + args.runs):
                    for who, net in (("fused", fused), ("stock", stock)):   # the candidates alternate
                        ms = timed(lambda: step(net, xx))
                        if it >= args.warmup:
                            t[who].append(ms)
                bwd, dx = label != "forward", label == "forward_backward_dx"
                nbytes = 4 * N * (D + L * F)
                if bwd:
                    nbytes += 4 * N * (D + L * F) + total * F * (4 + 8 + 8) + (4 * N * (D + L * F + D) if dx else 0)
                rec = dict(common, what=label, fused_ms=round(statistics.median(t["fused"]), 4), stock_ms=round(statistics.median(t["stock"]), 4),
                           floor_bytes_ms=round(nbytes / 8e12 * 1e3, 4))
                if bwd:
                    rec["floor_atomic_ms"] = round(N * L * (1 << D) * F * 8 / 1.3e12 * 1e3, 4)
                    xx.grad = table.grad = None
                    rec["fused_peak_mb"] = round(peak_above(lambda: fwd_bwd(fused, xx), 4 * N * L * F), 1)
                    xx.grad = table.grad = None
                    rec["stock_peak_mb"] = round(peak_above(lambda: fwd_bwd(stock, xx), 4 * N * L * F), 1)
                    for who, net in (("fused", fused), ("stock", stock)):
                        fwd_bwd(net, xx)
                        one = table.grad.clone()
                        fwd_bwd(net, xx)
                        rec[f"{who}_dtable_changes"] = not torch.equal(one, table.grad)
                    xx.grad = table.grad = None
                rec["speedup"] = round(rec["stock_ms"] / rec["fused_ms"], 3)
                emit(rec)
            # the raw backward's parts
            td = table.detach()
            d = fh.check(x, td, L, F, T, base, pls)
            rec = dict(common, what="table_backward", lds_levels=nlds, direct_levels=L - nlds,
                       table_ms=round(median_ms(lambda: fh._backward(d, x, td, g, False, True), args.runs, args.warmup), 4),
                       dx_ms=round(median_ms(lambda: fh._backward(d, x, td, g, True, False), args.runs, args.warmup), 4))
            if 0 < nlds < L:
                t_lds = td[:off[nlds]]
                d_lds = fh.check(x, t_lds, nlds, F, T, base, pls)
                rec["table_lds_ms"] = round(median_ms(lambda: fh._backward(d_lds, x, t_lds, g[:, :nlds * F], False, True), args.runs, args.warmup), 4)
                direct_ms = rec["table_ms"] - rec["table_lds_ms"]
                rec["added_tb_per_s"] = round(N * (L - nlds) * (1 << D) * F * 8 / (direct_ms * 1e-3) / 1e12, 3)
            emit(rec)
            del x, xg, g
            torch.cuda.empty_cache()
        del table
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
