"""Cost of the fused bilateral grid (include/gsr_bilagrid.h, fused_bilagrid.py) at 1980x1080 and 3840x2160 with the default grid
(12, 8, 16, 16):

  (i)   slice forward + backward (both gradients) against the same function in stock PyTorch fp32 with autograd -- a meshgrid, a
        matmul for the luma, a 5-D grid_sample over every pixel and twelve channels, a permute, a batched matmul -- on the same GPU
        in the same process;
  (ii)  the same against the streaming floor: the bytes that must move (forward: image in, image out; backward: image and dL/dout
        in, dL/dimage out; the grid and its gradient are 98 KB each) over 8 TB/s;
  (iii) the total variation of N = 200 grids, value and gradient, against the stock expression with autograd.

Every fused call goes straight to the C entry point with buffers allocated beforehand, so that the kernels are what is timed; wall
time between two events on the stream, the candidates alternated call by call in a rotating order, medians.  One JSON line, printed
and appended to profiles/bilagrid_bench.jsonl.

    python tools/bilagrid_bench.py --steps 30 --warmup 5
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "gaussian-splatting_cc-comments_amd"), os.path.join(R, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_BYTES_PER_S = 8e12


def stock_slice(grid, image):
    """gsplat's slice with pixel-centre coordinates, as a user writes it"""
    import torch
    import torch.nn.functional as F
    _, H, W = image.shape
    ys, xs = torch.meshgrid((torch.arange(H, device=image.device, dtype=image.dtype) + 0.5) / H,
                            (torch.arange(W, device=image.device, dtype=image.dtype) + 0.5) / W, indexing="ij")
    luma = torch.tensor([0.299, 0.587, 0.114], device=image.device, dtype=image.dtype) @ image.reshape(3, -1)
    coords = torch.stack([xs, ys, luma.reshape(H, W)], dim=-1) * 2 - 1
    A = F.grid_sample(grid[None], coords[None, None], mode="bilinear", align_corners=True, padding_mode="border")
    A = A[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
    rgb1 = torch.cat([image, torch.ones_like(image[:1])]).permute(1, 2, 0)
    return torch.matmul(A, rgb1[..., None])[..., 0].permute(2, 0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1980x1080,3840x2160")
    ap.add_argument("--tv-grids", type=int, default=200)
    ap.add_argument("--library", default=None, help="a variant build of libgsr_hip.so (csrc/Makefile, `make variant`) to run instead")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "bilagrid_bench.jsonl"))
    args = ap.parse_args()

    import torch

    import fused_bilagrid as fb
    import torch_bilagrid as ref
    from diff_gaussian_rasterization import _C
    if args.library:
        _C.use_library(os.path.abspath(args.library))
    dev = torch.device("cuda:0")
    lib = fb._lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    L, GH, GW = 8, 16, 16

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

    out = {"steps": args.steps, "warmup": args.warmup, "library": os.path.basename(args.library) if args.library else None, "grid": [12, L, GH, GW], "sizes": {}}
    g = torch.Generator().manual_seed(1)
    grid = (torch.eye(3, 4).reshape(12, 1, 1, 1) + 0.1 * torch.randn(12, L, GH, GW, generator=g)).to(dev)
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        x = torch.rand(3, H, W, generator=g).to(dev)
        go = torch.randn(3, H, W, generator=g).to(dev)
        o, dx, dg = torch.empty_like(x), torch.empty_like(x), torch.empty_like(grid)
        scratch = torch.empty(lib.gsr_bilagrid_scratch_bytes(H, W, L, GH, GW), dtype=torch.uint8, device=dev)
        a = fb.BilagridArgs(H=H, W=W, L=L, GH=GH, GW=GW, grid=grid.data_ptr(), img=x.data_ptr(), out=o.data_ptr(), dL_dout=go.data_ptr(),
                            dL_dgrid=dg.data_ptr(), dL_dimg=dx.data_ptr(), scratch=scratch.data_ptr(), stream=stream)

        a_grid = fb.BilagridArgs.from_buffer_copy(a)
        a_grid.dL_dimg = None
        a_image = fb.BilagridArgs.from_buffer_copy(a)
        a_image.dL_dgrid = None

        def fused_backward_grid():
            check(lib.gsr_bilagrid_slice_backward(ctypes.byref(a_grid)))

        def fused_backward_image():
            check(lib.gsr_bilagrid_slice_backward(ctypes.byref(a_image)))

        def fused_forward():
            check(lib.gsr_bilagrid_slice(ctypes.byref(a)))

        def fused():
            check(lib.gsr_bilagrid_slice(ctypes.byref(a)))
            check(lib.gsr_bilagrid_slice_backward(ctypes.byref(a)))

        def stock():
            gs, xs = grid.detach().clone().requires_grad_(True), x.detach().clone().requires_grad_(True)
            stock_slice(gs, xs).backward(go)
            return gs.grad, xs.grad

        # the two compute the same thing (fp32 against fp32; grid_sample's backward adds with atomics)
        fused()
        sg, sx = stock()
        agree = {"out": float((o - stock_slice(grid, x)).abs().max()), "dgrid_rel": float((dg - sg).abs().max() / sg.abs().max()),
                 "dimage_rel": float((dx - sx).abs().max() / sx.abs().max())}
        med = medians({"fused": fused, "fused_forward": fused_forward, "fused_backward_grid": fused_backward_grid,
                       "fused_backward_image": fused_backward_image, "stock": stock})
        plane = 3 * H * W * 4
        floor_ms = (2 * plane + 3 * plane) / HBM_BYTES_PER_S * 1e3
        out["sizes"][size] = {"i_fused_fwd_bwd_ms": round(med["fused"], 4), "i_fused_fwd_ms": round(med["fused_forward"], 4),
                              "i_fused_bwd_grid_ms": round(med["fused_backward_grid"], 4), "i_fused_bwd_image_ms": round(med["fused_backward_image"], 4),
                              "i_stock_pytorch_fwd_bwd_ms": round(med["stock"], 4), "i_stock_over_fused": round(med["stock"] / med["fused"], 2),
                              "ii_streaming_floor_ms": round(floor_ms, 4), "ii_fused_over_floor": round(med["fused"] / floor_ms, 2),
                              "agreement_with_stock_fp32": agree}

    N = args.tv_grids
    grids = (torch.eye(3, 4).reshape(1, 12, 1, 1, 1) + 0.1 * torch.randn(N, 12, L, GH, GW, generator=g)).to(dev)
    val, dgrids = torch.empty(1, device=dev), torch.empty_like(grids)
    scratch = torch.empty(lib.gsr_bilagrid_tv_scratch_bytes(N, L, GH, GW), dtype=torch.uint8, device=dev)

    def fused_tv():
        check(lib.gsr_bilagrid_tv(N, L, GH, GW, grids.data_ptr(), val.data_ptr(), dgrids.data_ptr(), scratch.data_ptr(), stream))

    def stock_tv():
        gs = grids.detach().clone().requires_grad_(True)
        tv = ref.total_variation(gs)
        tv.backward()
        return tv.detach(), gs.grad

    fused_tv()
    tv, sgrad = stock_tv()
    med = medians({"fused": fused_tv, "stock": stock_tv})
    floor_ms = 2 * grids.numel() * 4 / HBM_BYTES_PER_S * 1e3
    out["tv"] = {"N": N, "iii_fused_ms": round(med["fused"], 4), "iii_stock_pytorch_ms": round(med["stock"], 4),
                 "iii_stock_over_fused": round(med["stock"] / med["fused"], 2), "streaming_floor_ms": round(floor_ms, 4),
                 "agreement_with_stock_fp32": {"value_rel": abs(float(val) - float(tv)) / float(tv),
                                               "grad_rel": float((dgrids - sgrad).abs().max() / sgrad.abs().max())}}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
