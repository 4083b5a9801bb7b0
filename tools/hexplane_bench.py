"""The fused plane-grid encoding (fused_hexplane.hex_plane) against the stock float32 torch version with autograd (six F.grid_sample
calls per level, the products kept by autograd, a backward that scatters into the planes with float atomics), on the same GPU in the
same process.

    python tools/hexplane_bench.py [--shapes ...] [--rows 1000000] [--runs 30] [--warmup 5] [--out profiles/hexplane_bench.jsonl]

Buffers are allocated beforehand; a run's wall time is taken between two events; the two candidates alternate run by run; the
figure is the median of --runs runs after --warmup.  One JSON line per shape, row count and pass (forward; forward + backward with and
without dx; the regulariser with its gradient) with
  fused_ms, stock_ms, speedup      the two medians and stock / fused
  floor_bytes_ms                   the bytes that must stream (x, y; backward: x again, dy, the table read once for its maxima, dtable,
                                   the scratch sums written by the clear and read by the convert, dx) over 8 TB/s
  floor_requests_ms                backward: the integer adds, N L P 4 C, as 64-byte requests of 8 adds each, over 23 G requests/s (the
                                   rate section 6za measured for scattered 64-bit integer adds, one request each)
  fused_peak_mb, stock_peak_mb     peak memory during one forward + backward above the inputs and the outputs
  stock_dtable_changes, fused_dtable_changes   whether dtable differs between two runs
and, once per shape and row count (what = "table_backward"), the raw backward's parts:
  lds_planes, direct_planes        how many planes take which path
  table_ms                         the backward for dtable alone
  lds_ms, direct_ms                of which the LDS-path kernel and the direct-path kernel (their own dispatch timestamps, summed over
                                   the passes; medians of --runs calls)
  direct_gadds_per_s               the direct planes' adds, N (direct planes) 4 C, over direct_ms
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
import fused_hexplane as fh  # noqa: E402
import torch_hexplane as th  # noqa: E402
from diff_gaussian_rasterization import _C  # noqa: E402

# (D, C, base, multires), default rows
SHAPES = {
    "d4_c16_t150_x2": ((4, 16, (64, 64, 64, 150), (1, 2)), [1000000, 6000000]),
    "d4_c32_t25_x8": ((4, 32, (64, 64, 64, 25), (1, 2, 4, 8)), [1000000, 6000000]),
    "d3_c32_x4": ((3, 32, (64, 64, 64), (1, 2, 4)), [1000000, 6000000]),
}
REG = dict(tv_space=2e-4, tv_time=2e-4, smooth_time=1e-3, l1_time=1e-4)


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


def stage_ms(fn, stage, runs, warmup):
    """The median over `runs` calls of the summed time of one single-kernel stage"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        _C.profile_begin(only=stage)
        fn()
        out.append(sum(ms for _, ms in _C.profile_end()))
    return statistics.median(out)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hexplane_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def emit(rec):
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")

    for name in args.shapes:
        (D, C, base, multires), rows = SHAPES[name]
        cfg = fh.HexPlaneConfig(D, C, fh.resolutions(base, multires), True)
        tcfg = th.Cfg(D, C, cfg.res, True)
        L, P, total = cfg.levels, len(cfg.planes), cfg.total()
        paths = [p for level in fh.level_paths(cfg) for p in level]
        nlds = sum(p == fh.PATH_LDS for p in paths)
        table = (torch.rand(total, device=dev) * 0.4 + 0.1).requires_grad_(True)
        common = dict(shape=name, D=D, C=C, res=[list(r) for r in cfg.res], table_floats=total, runs=args.runs, pid=os.getpid())
        # the regulariser: value and gradient
        def reg(f):
            table.grad = None
            f().backward()
        t = {"fused": [], "stock": []}
        for it in range(args.warmup + args.runs):
            for who, f in (("fused", lambda: fh.plane_regularizer(table, cfg, **REG)), ("stock", lambda: th.regularizer_torch(table, tcfg, **REG))):
                ms = timed(lambda: reg(f))
                if it >= args.warmup:
                    t[who].append(ms)
        rec = dict(common, what="regularizer", fused_ms=round(statistics.median(t["fused"]), 4), stock_ms=round(statistics.median(t["stock"]), 4),
                   floor_bytes_ms=round(total * 8 / 8e12 * 1e3, 4))
        rec["speedup"] = round(rec["stock_ms"] / rec["fused_ms"], 3)
        emit(rec)
        table.grad = None
        for N in args.rows or rows:
            x = torch.rand((N, D), device=dev) * 2 - 1
            xg = x.clone().requires_grad_(True)
            g = torch.randn((N, L * C), device=dev)
            fused = lambda xx: fh.hex_plane(xx, table, cfg)
            stock = lambda xx: th.hex_plane_torch(xx, table, tcfg)

            def fwd(net, xx):
                with torch.no_grad():
                    return net(xx)

            def fwd_bwd(net, xx):
                xx.grad = None
                table.grad = None
                net(xx).backward(g)

            for label, step, xx in (("forward", fwd, x), ("forward_backward_dx", fwd_bwd, xg), ("forward_backward", fwd_bwd, x)):
                t = {"fused": [], "stock": []}
                for it in range(args.warmup + args.runs):
                    for who, net in (("fused", fused), ("stock", stock)):   # the candidates alternate
                        ms = timed(lambda: step(net, xx))
                        if it >= args.warmup:
                            t[who].append(ms)
                bwd, dx = label != "forward", label == "forward_backward_dx"
                nbytes = 4 * N * (D + L * C)
                if bwd:
                    nbytes += 4 * N * (D + L * C) + total * (4 + 4 + 8 + 8) + (4 * N * (D + L * C + D) if dx else 0)
                rec = dict(common, rows=N, what=label, fused_ms=round(statistics.median(t["fused"]), 4), stock_ms=round(statistics.median(t["stock"]), 4),
                           floor_bytes_ms=round(nbytes / 8e12 * 1e3, 4))
                if bwd:
                    rec["floor_requests_ms"] = round(N * L * P * 4 * C / 8 / 23e9 * 1e3, 4)
                    xx.grad = table.grad = None
                    rec["fused_peak_mb"] = round(peak_above(lambda: fwd_bwd(fused, xx), 4 * N * L * C), 1)
                    xx.grad = table.grad = None
                    rec["stock_peak_mb"] = round(peak_above(lambda: fwd_bwd(stock, xx), 4 * N * L * C), 1)
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
            d = fh.check(x, td, cfg)
            only_table = lambda: fh._backward(d, x, td, g, False, True)
            rec = dict(common, rows=N, what="table_backward", lds_planes=nlds, direct_planes=L * P - nlds,
                       table_ms=round(median_ms(only_table, args.runs, args.warmup), 4),
                       dx_ms=round(median_ms(lambda: fh._backward(d, x, td, g, True, False), args.runs, args.warmup), 4),
                       lds_ms=round(stage_ms(only_table, "hexplane_backward_lds", args.runs, 1), 4),
                       direct_ms=round(stage_ms(only_table, "hexplane_backward_direct", args.runs, 1), 4))
            if rec["direct_ms"] > 0:
                rec["direct_gadds_per_s"] = round(N * (L * P - nlds) * 4 * C / (rec["direct_ms"] * 1e-3) / 1e9, 2)
            emit(rec)
            del x, xg, g
            torch.cuda.empty_cache()
        del table
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
