"""Cost of the fused neighbour-rigidity losses (include/gsr_rigidity.h, fused_rigidity.py) on the `clustered` cloud of
tools/knn_bench.py: value + both gradients at --sizes points and --ks neighbours, against what a user has on the same GPU in the same
process:

  (i)   the stock float32 PyTorch sequence of Dynamic 3D Gaussians' get_loss with autograd, neighbours through x[idx.long()];
  (ii)  the same sequence with neighbours through fused_knn.neighbor_gather;
  (iii) the streaming floor of the bytes that must move: the tables read once (24 bytes per edge), 28 bytes written and read per
        edge, the leaves, the captured rotations and the gradients once (72 bytes per point), at --floor-tbs TB/s.

The stock sequence forms R^T c as a broadcast product and a sum, not as the paper's `rot.transpose(2, 1)[:, None] @ c[..., None]`: on
the PyTorch-ROCm build this was written on, that batched matrix product over P K = 20M three-by-three matrices took 0.6 s per step
and the loss that came out of it was 1.5 % away from the fused one (the broadcast form: 1e-7 per term), so it is no yardstick.
--float64-check also runs the sequence in float64 on the device and reports how far each side's gradients are from it.

The fused side goes straight to the C entry point with every buffer allocated beforehand, so that the kernels are what is timed; wall
time between two events on the stream, the candidates alternated call by call in a rotating order, medians.  Peak memory above the
inputs (leaves and state) is torch's peak of allocated bytes over one call of each candidate through its Python surface.  The
measurement runs in two fresh processes one after the other; one JSON line per process, printed and appended to
profiles/rigidity_bench.jsonl.

    python tools/rigidity_bench.py --steps 10 --warmup 2
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "gaussian-splatting_cc-comments_amd"), os.path.join(R, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def child(args):
    import torch

    from diff_gaussian_rasterization import _C
    if args.library:
        _C.use_library(os.path.abspath(args.library))
    import fused_knn as fk
    import fused_rigidity as fr
    from knn_bench import clustered
    dev = torch.device("cuda:0")
    lib = fr._lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    lam = (4.0, 4.0, 2.0)

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

    def peak_above(f):   # allocated, not reserved, bytes: the allocator's cache is left as it is
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        keep = f()
        torch.cuda.synchronize(dev)
        peak = torch.cuda.max_memory_allocated(dev) - base
        del keep
        return peak

    def quat_mult(q1, q2):
        w1, x1, y1, z1 = q1.T
        w2, x2, y2, z2 = q2.T
        return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                            w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2]).T

    def build_rotation(q):
        q = torch.nn.functional.normalize(q)
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        rot = torch.zeros((q.size(0), 3, 3), device=q.device, dtype=q.dtype)
        rot[:, 0, 0] = 1 - 2 * (y * y + z * z); rot[:, 0, 1] = 2 * (x * y - r * z); rot[:, 0, 2] = 2 * (x * z + r * y)
        rot[:, 1, 0] = 2 * (x * y + r * z); rot[:, 1, 1] = 1 - 2 * (x * x + z * z); rot[:, 1, 2] = 2 * (y * z - r * x)
        rot[:, 2, 0] = 2 * (x * z - r * y); rot[:, 2, 1] = 2 * (y * z + r * x); rot[:, 2, 2] = 1 - 2 * (x * x + y * y)
        return rot

    def l2_v1(x, y, w):
        return torch.sqrt(((x - y) ** 2) * w + 1e-20).mean()

    def l2_v2(x, y, w):
        return torch.sqrt(((x - y) ** 2).sum(-1) * w + 1e-20).mean()

    out = {"steps": args.steps, "warmup": args.warmup, "library": os.path.basename(args.library) if args.library else None,
           "floor_tbs": args.floor_tbs, "cases": {}}
    for P in (int(v) for v in args.sizes.split(",")):
        pts = torch.from_numpy(clustered(P, 11)).to(dev)
        g = torch.Generator(device=dev).manual_seed(5)
        rot0 = torch.nn.functional.normalize(torch.randn(P, 4, device=dev, generator=g))
        for K in (int(v) for v in args.ks.split(",")):
            state = fr.RigidityState.capture(pts, rot0, K, weight_lambda=args.weight_lambda)
            capture_ms = timed(lambda: fr.RigidityState.capture(pts, rot0, K, weight_lambda=args.weight_lambda))
            d1 = state.prev_dist[:, :1]
            xyz = (pts + 0.1 * d1 * torch.randn(P, 3, device=dev, generator=g)).contiguous()   # a tenth of the nearest neighbour's distance
            rot = rot0 + 0.05 * torch.randn(P, 4, device=dev, generator=g)
            values, gx, gr = torch.empty(4, device=dev), torch.empty(P, 3, device=dev), torch.empty(P, 4, device=dev)
            scratch = torch.empty(lib.gsr_rigidity_scratch_bytes(P, K), dtype=torch.uint8, device=dev)
            s, gph = state, state.graph

            def fused(gxp=gx.data_ptr(), grp=gr.data_ptr()):
                rc = lib.gsr_rigidity_loss(P, K, xyz.data_ptr(), rot.data_ptr(), s.idx.data_ptr(), s.prev_offset.data_ptr(), s.prev_dist.data_ptr(),
                                           s.weight.data_ptr(), s.prev_inv_rot.data_ptr(), gph.offsets.data_ptr(), gph._edges.data_ptr(), *lam,
                                           values.data_ptr(), gxp, grp, scratch.data_ptr(), stream)
                assert rc == 0, lib.gsr_last_error()

            def fused_value_only():
                fused(None, None)

            long_idx = s.idx.long()

            def stock(gather, dtype=torch.float32):
                x, r = xyz.detach().to(dtype).requires_grad_(True), rot.detach().to(dtype).requires_grad_(True)
                prev_inv_rot, prev_offset, prev_dist, weight = (t.to(dtype) for t in (s.prev_inv_rot, s.prev_offset, s.prev_dist, s.weight))
                q = torch.nn.functional.normalize(r)
                rel = quat_mult(q, prev_inv_rot)
                rmat = build_rotation(rel)
                nb = gather(x)
                c = nb - x[:, None]
                u = (rmat[:, None] * c[:, :, :, None]).sum(-2)   # R^T c as a broadcast product (see the note above)
                terms = (l2_v2(u, prev_offset, weight), l2_v2(gather(rel), rel[:, None], weight),
                         l2_v1(torch.sqrt((c ** 2).sum(-1) + 1e-20), prev_dist, weight))
                loss = lam[0] * terms[0] + lam[1] * terms[1] + lam[2] * terms[2]
                loss.backward()
                return loss.detach(), x.grad, r.grad, torch.stack(terms).detach()

            def stock_index():
                return stock(lambda t: t[long_idx])

            def stock_gather():
                return stock(lambda t: fk.neighbor_gather(t, gph))

            fused()
            if args.fused_only:   # a variant of the kernels against another: no stock candidates
                med = medians({"fused": fused, "fused_value_only": fused_value_only})
                out["cases"][f"{P}x{K}"] = {"N_e": state.num_edges, "fused_ms": round(med["fused"], 3), "fused_value_only_ms": round(med["fused_value_only"], 3)}
                continue
            ref = stock_index()
            scale_x, scale_r = float(ref[1].abs().max()), float(ref[2].abs().max())
            agree = {"loss_rel": abs(float(values[0]) - float(ref[0])) / abs(float(ref[0])),
                     "terms_rel": [abs(float(values[1 + k]) - float(ref[3][k])) / abs(float(ref[3][k])) for k in range(3)],
                     "grad_xyz_max_abs_over_max": float((gx - ref[1]).abs().max()) / scale_x,
                     "grad_rot_max_abs_over_max": float((gr - ref[2]).abs().max()) / scale_r,
                     "grad_xyz_l2_over_l2": float((gx - ref[1]).double().norm() / ref[1].double().norm()),
                     "grad_rot_l2_over_l2": float((gr - ref[2]).double().norm() / ref[2].double().norm()),
                     "grad_xyz_rows_off_by_more_than_1e-3_of_max": int(((gx - ref[1]).abs().amax(dim=1) > 1e-3 * scale_x).sum())}
            if args.float64_check:   # which side a disagreement belongs to: the same sequence in float64 on the device
                r64 = stock(lambda t: t[long_idx], torch.float64)

                def against(g, want):
                    diff, top = (g.double() - want), float(want.abs().max())
                    return {"max_abs_over_max": float(diff.abs().max()) / top, "l2_over_l2": float(diff.norm() / want.norm()),
                            "rows_off_by_more_than_1e-3_of_max": int((diff.abs().amax(dim=1) > 1e-3 * top).sum())}

                agree["float64_check"] = {"fused_grad_xyz": against(gx, r64[1]), "stock_index_grad_xyz": against(ref[1], r64[1]),
                                          "fused_grad_rot": against(gr, r64[2]), "stock_index_grad_rot": against(ref[2], r64[2]),
                                          "fused_loss_rel": abs(float(values[0]) - float(r64[0])) / float(r64[0]),
                                          "stock_index_loss_rel": abs(float(ref[0]) - float(r64[0])) / float(r64[0])}
                del r64
            del ref
            med = medians({"fused": fused, "fused_value_only": fused_value_only, "stock_index": stock_index, "stock_gather": stock_gather})
            print(f"{P}x{K}: medians {med}", file=sys.stderr, flush=True)
            del scratch
            mem = {"fused": peak_above(lambda: fr.rigidity_loss_and_grads(xyz, rot, state)),
                   "stock_index": peak_above(stock_index), "stock_gather": peak_above(stock_gather)}
            E = state.num_edges
            floor_bytes = (24 + 56) * E + 72 * P
            floor_ms = floor_bytes / (args.floor_tbs * 1e12) * 1e3
            in_deg = (gph.offsets[1:] - gph.offsets[:-1])
            out["cases"][f"{P}x{K}"] = {
                "N_e": E, "capture_ms": round(capture_ms, 3), "max_in_degree": int(in_deg.max()),
                "fused_ms": round(med["fused"], 3), "fused_value_only_ms": round(med["fused_value_only"], 3),
                "stock_index_ms": round(med["stock_index"], 3), "stock_gather_ms": round(med["stock_gather"], 3),
                "stock_index_over_fused": round(med["stock_index"] / med["fused"], 2), "stock_gather_over_fused": round(med["stock_gather"] / med["fused"], 2),
                "floor_bytes": floor_bytes, "floor_ms": round(floor_ms, 3), "fused_over_floor": round(med["fused"] / floor_ms, 2),
                "peak_bytes_above_inputs": mem, "agreement_with_stock_index": agree}
            print(f"{P}x{K}: {json.dumps(out['cases'][f'{P}x{K}'])}", file=sys.stderr, flush=True)
            del state, s, gph, long_idx, values, gx, gr, xyz, rot
        del pts, rot0
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
    ap.add_argument("--ks", default="20,16")
    ap.add_argument("--weight-lambda", type=float, default=2000.0)
    ap.add_argument("--floor-tbs", type=float, default=6.0, help="the streaming rate the floor is priced at, TB/s")
    ap.add_argument("--float64-check", action="store_true", help="also compare both sides' gradients with the stock sequence in float64 on the device")
    ap.add_argument("--fused-only", action="store_true", help="time the fused calls alone (A/B of kernel variants)")
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--library", default=None, help="a variant build of libgsr_hip.so (csrc/Makefile, `make variant`) to run instead")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "rigidity_bench.jsonl"))
    ap.add_argument("--child", action="store_true", help="measure in this process (what the tool starts --processes times)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    for _ in range(args.processes):   # fresh processes, one after the other; this one never opens the device
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"], check=True)


if __name__ == "__main__":
    main()
