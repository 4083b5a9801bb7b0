"""Cost of the neighbour graph (include/gsr_knn.h, fused_knn.py) on the `clustered` cloud of tests/test_knn.py, against what a user has
on the same GPU in the same process:

  search   K = 3, 16 and 32 at 1M and 6M points (self-set form), against
           (a) distCUDA2 (gsr_knn_mean_dist2) for K = 3: the same traversal with three distances and no indices;
           (b) a chunked torch.cdist + topk.  A full pass is 10^12 distance evaluations at 1M points, so it is timed on
               --cdist-queries queries in chunks of --cdist-chunk and scaled to all of them (reported as extrapolated);
  graph    the reverse adjacency of the K = 16 table;
  gather   forward + backward at C = 3 and 48 over the K = 16 table, against (c) x[idx.long()] with autograd, whose backward
           scatters with float atomics.
  one target: the backward of --one-target-edges edges that all point at row 0 (C = 3), the longest sequential sum there is.
  --scipy  also scipy's cKDTree on the host cores (K = 3, up to 1M points), the CPU fallback of other code bases.

Every fused call goes straight to the C entry point with buffers allocated beforehand, so that the kernels are what is timed; wall
time between two events on the stream, the candidates alternated call by call in a rotating order, medians.  The measurement runs in
two fresh processes one after the other; one JSON line per process, printed and appended to profiles/knn_bench.jsonl.

    python tools/knn_bench.py --steps 10 --warmup 2
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


def clustered(P, seed):
    """tests/test_knn.py _cloud(P, seed, "clustered")"""
    import numpy as np
    r = np.random.default_rng(seed)
    c = r.normal(size=(max(P // 200, 1), 3)) * 4
    pts = c[r.integers(0, len(c), P)] + r.normal(size=(P, 3)) * r.choice([0.01, 0.1, 1.0], size=(P, 1))
    return pts.astype(np.float32)


def child(args):
    import torch

    import fused_knn as fk
    from diff_gaussian_rasterization import _C
    from simple_knn._C import distCUDA2
    if args.library:
        _C.use_library(os.path.abspath(args.library))
    dev = torch.device("cuda:0")
    lib = fk._lib()
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

    out = {"steps": args.steps, "warmup": args.warmup, "library": os.path.basename(args.library) if args.library else None, "search": {},
           "graph": {}, "gather": {}}
    for P in (int(v) for v in args.sizes.split(",")):
        pts = torch.from_numpy(clustered(P, 11)).to(dev)
        distCUDA2(pts[:1000])   # binds gsr_knn_mean_dist2
        mean = torch.empty(P, device=dev)
        scratch3 = torch.empty(lib.gsr_knn_scratch_bytes(P), dtype=torch.uint8, device=dev)
        scratch = torch.empty(lib.gsr_knn_search_scratch_bytes(P, 0), dtype=torch.uint8, device=dev)
        bufs = {K: (torch.empty(P, K, device=dev), torch.empty(P, K, dtype=torch.int32, device=dev)) for K in (3, 16, 32)}

        def search(K):
            d, i = bufs[K]
            return lambda: check(lib.gsr_knn_search(P, pts.data_ptr(), P, None, K, d.data_ptr(), i.data_ptr(), scratch.data_ptr(), stream))

        def dist3():
            check(lib.gsr_knn_mean_dist2(P, pts.data_ptr(), mean.data_ptr(), scratch3.data_ptr(), stream))

        nq, chunk = min(args.cdist_queries, P), args.cdist_chunk

        def cdist_topk(K):
            def run():
                for lo in range(0, nq, chunk):
                    d = torch.cdist(pts[lo:lo + chunk], pts)
                    d.topk(K + 1, dim=1, largest=False)   # the point itself + K others
            return run

        med = medians({"k3": search(3), "k16": search(16), "k32": search(32), "distCUDA2": dist3})
        d3 = bufs[3][0]
        same = bool(torch.equal(((d3[:, 0] + d3[:, 1]) + d3[:, 2]) / torch.full_like(mean, 3.0), mean))   # a tensor divisor: a true division
        cd = medians({f"k{K}": cdist_topk(K) for K in (3, 16, 32)}, steps=args.cdist_steps, warmup=1)
        row = {"distCUDA2_ms": round(med["distCUDA2"], 3), "k3_mean_has_distCUDA2_bits": same, "k3_over_distCUDA2": round(med["k3"] / med["distCUDA2"], 3),
               "cdist_queries_timed": nq, "cdist_chunk": chunk}
        for K in (3, 16, 32):
            full = cd[f"k{K}"] * (P / nq)
            row[f"k{K}_ms"] = round(med[f"k{K}"], 3)
            row[f"k{K}_cdist_topk_ms_extrapolated"] = round(full, 1)
            row[f"k{K}_cdist_topk_over_fused"] = round(full / med[f"k{K}"], 1)
        if args.scipy and P <= 1000000:   # what the CPU fallback of other code bases costs: scipy's k-d tree on the host cores, K = 3
            import time

            from scipy.spatial import cKDTree
            host = pts.cpu().numpy()
            t0 = time.perf_counter()
            cKDTree(host).query(host, k=4, workers=-1)
            row["scipy_ckdtree_k3_host_s"] = round(time.perf_counter() - t0, 2)
        out["search"][str(P)] = row

        idx = bufs[16][1]
        E = P * 16
        offsets = torch.empty(P + 1, dtype=torch.int32, device=dev)
        edges = torch.empty(E, dtype=torch.int32, device=dev)
        gscratch = torch.empty(lib.gsr_knn_graph_scratch_bytes(E, P), dtype=torch.uint8, device=dev)

        def build():
            check(lib.gsr_knn_graph_build(E, idx.data_ptr(), P, offsets.data_ptr(), edges.data_ptr(), None, gscratch.data_ptr(), stream))

        build()
        out["graph"][str(P)] = {"K": 16, "build_ms": round(medians({"build": build})["build"], 3)}
        del gscratch, scratch, scratch3
        long_idx = idx.long()
        for C in (3, 48):
            x = torch.randn(P, C, device=dev)
            o, go, gx = torch.empty(P, 16, C, device=dev), torch.randn(P, 16, C, device=dev), torch.empty(P, C, device=dev)

            def fused():
                check(lib.gsr_knn_gather(P, 16, C, x.data_ptr(), idx.data_ptr(), o.data_ptr(), stream))
                check(lib.gsr_knn_gather_backward(P, C, offsets.data_ptr(), edges.data_ptr(), go.data_ptr(), gx.data_ptr(), stream))

            def stock():
                t = x.detach().requires_grad_(True)
                t[long_idx].backward(go)
                return t.grad

            fused()
            a, b = stock(), stock()
            med = medians({"fused": fused, "stock": stock})
            out["gather"][f"{P}x{C}"] = {"K": 16, "fused_fwd_bwd_ms": round(med["fused"], 3), "stock_index_autograd_ms": round(med["stock"], 3),
                                         "stock_over_fused": round(med["stock"] / med["fused"], 2),
                                         "stock_two_runs_same_bits": bool(torch.equal(a, b)),
                                         "max_abs_diff_to_stock": float((gx - a).abs().max())}
            del x, o, go, gx, a, b
        del long_idx, bufs, pts
        torch.cuda.empty_cache()
    # the worst row for the backward: every one of E edges on one target, a sequential sum of E terms per channel
    E, C = args.one_target_edges, 3
    idx = torch.zeros(E // 16, 16, dtype=torch.int32, device=dev)
    g = fk.NeighborGraph(idx, 1)
    go, gx = torch.randn(E // 16, 16, C, device=dev), torch.empty(1, C, device=dev)

    def one_target():
        check(lib.gsr_knn_gather_backward(1, C, g.offsets.data_ptr(), g._edges.data_ptr(), go.data_ptr(), gx.data_ptr(), stream))

    out["one_target_backward"] = {"E": E, "C": C, "ms": round(medians({"b": one_target}, steps=3, warmup=1)["b"], 2)}
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
    ap.add_argument("--cdist-queries", type=int, default=4096)
    ap.add_argument("--cdist-chunk", type=int, default=1024)
    ap.add_argument("--cdist-steps", type=int, default=3)
    ap.add_argument("--one-target-edges", type=int, default=16000000)
    ap.add_argument("--scipy", action="store_true", help="also time scipy's cKDTree on the host cores at up to 1M points")
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--library", default=None, help="a variant build of libgsr_hip.so (csrc/Makefile, `make variant`) to run instead")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "knn_bench.jsonl"))
    ap.add_argument("--child", action="store_true", help="measure in this process (what the tool starts --processes times)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    for _ in range(args.processes):   # fresh processes, one after the other; this one never opens the device
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"], check=True)


if __name__ == "__main__":
    main()
