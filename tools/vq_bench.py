"""Cost of the vector quantisation (include/gsr_vq.h, fused_vq.py) on Gaussian rows, against what a user has on the same GPU in the
same process:

  assign   N = 1M and 6M rows, D = 45 and D = 7, K = 4096, against
           (a) the stock float32 sequence: in chunks of --stock-chunk rows |x|^2 - 2 x c^T + |c|^2 -> argmin (an N x K matrix written
               and read back, chunk by chunk);
           (b) the floor 2 N K D_padded flops at the fp32-MFMA peak (--peak-tflops), D_padded = the k steps the kernel issues;
  update   the graph build plus the centroid kernel, against (c) index_add_ (float atomics) and a divide;
  kmeans   one whole Lloyd iteration of fused_vq.kmeans (assign, inertia, graph build, update), by the difference of a 3- and a
           1-iteration call.

The fused entry points are called directly with buffers allocated beforehand; wall time between two events on the stream, the
candidates alternated call by call in a rotating order, medians.  peak_extra_mib is the allocator's peak above the inputs over the
fused assign and update.  The measurement runs in two fresh processes one after the other; one JSON line per process, printed and
appended to profiles/vq_bench.jsonl.

    python tools/vq_bench.py --steps 10 --warmup 2
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


def padded_d(D):
    """csrc/vq.hip gsr_vq_ksteps: twice the k steps of the instantiation that holds D"""
    return 2 * (4 if D <= 8 else 8 if D <= 16 else 16 if D <= 32 else 24 if D <= 48 else 32)


def child(args):
    import torch

    import fused_knn as fk
    import fused_vq as fv
    from diff_gaussian_rasterization import _C
    if args.library:
        _C.use_library(os.path.abspath(args.library))
    dev = torch.device("cuda:0")
    lib = fv._lib()
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

    K = args.codes
    out = {"steps": args.steps, "warmup": args.warmup, "library": os.path.basename(args.library) if args.library else None, "K": K,
           "peak_tflops": args.peak_tflops, "cases": {}}
    for N in (int(v) for v in args.sizes.split(",")):
        for D in (int(v) for v in args.dims.split(",")):
            g = torch.Generator(device=dev).manual_seed(N + D)
            x = torch.randn(N, D, device=dev, generator=g)
            w = torch.rand(N, device=dev, generator=g)
            cb = x[torch.randperm(N, device=dev, generator=g)[:K]].contiguous()
            idx, d2 = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, device=dev)
            scratch = torch.empty(lib.gsr_vq_assign_scratch_bytes(N, D, K), dtype=torch.uint8, device=dev)
            offsets, members = torch.empty(K + 1, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
            gscratch = torch.empty(lib.gsr_knn_graph_scratch_bytes(N, K), dtype=torch.uint8, device=dev)
            new, count, wsum = cb.clone(), torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, device=dev)

            def assign():
                check(lib.gsr_vq_assign(N, D, x.data_ptr(), K, cb.data_ptr(), idx.data_ptr(), d2.data_ptr(), scratch.data_ptr(), stream))

            def update():
                check(lib.gsr_knn_graph_build(N, idx.data_ptr(), K, offsets.data_ptr(), members.data_ptr(), None, gscratch.data_ptr(), stream))
                check(lib.gsr_vq_update(N, D, x.data_ptr(), w.data_ptr(), K, offsets.data_ptr(), members.data_ptr(), new.data_ptr(), count.data_ptr(),
                                        wsum.data_ptr(), stream))

            sidx = torch.empty(N, dtype=torch.int64, device=dev)

            def stock_assign():
                c2 = (cb * cb).sum(1)
                for lo in range(0, N, args.stock_chunk):
                    xc = x[lo:lo + args.stock_chunk]
                    s = (xc * xc).sum(1, keepdim=True) - 2.0 * (xc @ cb.t()) + c2
                    sidx[lo:lo + args.stock_chunk] = s.argmin(1)

            def stock_update():
                S = torch.zeros(K, D, device=dev).index_add_(0, sidx, x * w[:, None])
                W = torch.zeros(K, device=dev).index_add_(0, sidx, w)
                return S / W.clamp_min(1e-30)[:, None]

            torch.cuda.synchronize(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            assign(); update()
            torch.cuda.synchronize(dev)
            extra = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20   # 0: the calls allocate nothing; the buffers are counted below
            held = sum(t.numel() * t.element_size() for t in (idx, d2, scratch, offsets, members, gscratch, new, count, wsum)) / 2 ** 20
            stock_assign()
            a, b = stock_update(), stock_update()
            med = medians({"assign": assign, "update": update, "stock_assign": stock_assign, "stock_update": stock_update})
            km = medians({"k1": lambda: fv.kmeans(x, K, iters=1, init=cb, weight=w), "k3": lambda: fv.kmeans(x, K, iters=3, init=cb, weight=w)},
                         steps=max(3, args.steps // 3), warmup=1)
            floor = 2.0 * N * K * padded_d(D) / (args.peak_tflops * 1e12) * 1e3
            out["cases"][f"{N}x{D}"] = {
                "assign_ms": round(med["assign"], 3), "floor_ms": round(floor, 3), "assign_over_floor": round(med["assign"] / floor, 2),
                "assign_tflops_padded": round(2.0 * N * K * padded_d(D) / med["assign"] / 1e9, 1),
                "stock_assign_ms": round(med["stock_assign"], 3), "stock_assign_over_fused": round(med["stock_assign"] / med["assign"], 2),
                "update_ms": round(med["update"], 3), "stock_update_ms": round(med["stock_update"], 3),
                "stock_update_over_fused": round(med["stock_update"] / med["update"], 2),
                "stock_update_two_runs_same_bits": bool(torch.equal(a, b)),
                "agree_with_stock_argmin": round(float((idx.long() == sidx).float().mean()), 6),
                "kmeans_iteration_ms": round((km["k3"] - km["k1"]) / 2, 3),
                "fused_buffers_mib": round(held, 1), "peak_extra_mib": round(extra, 1)}
            del x, w, cb, idx, d2, scratch, offsets, members, gscratch, new, count, wsum, sidx, a, b
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1000000,6000000")
    ap.add_argument("--dims", default="45,7")
    ap.add_argument("--codes", type=int, default=4096)
    ap.add_argument("--stock-chunk", type=int, default=65536, help="rows per chunk of the stock sequence (65536 x 4096 floats = 1 GiB)")
    ap.add_argument("--peak-tflops", type=float, default=157.3, help="fp32-input MFMA peak of the device")
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--library", default=None, help="a variant build of libgsr_hip.so (csrc/Makefile, `make variant`) to run instead")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "vq_bench.jsonl"))
    ap.add_argument("--child", action="store_true", help="measure in this process (what the tool starts --processes times)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    for _ in range(args.processes):   # fresh processes, one after the other; this one never opens the device
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"], check=True)


if __name__ == "__main__":
    main()
