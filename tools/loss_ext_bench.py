"""Cost of the extended fused loss (include/gsr_loss_ext.h, fused_loss.training_loss*), forward plus backward, at 1980x1080 and
3840x2160:

  (a) gsr_l1_ssim_loss_ext with every option (mask, exposure, inverse-depth term with its mask) and every gradient;
  (b) gsr_l1_ssim_loss_ext with no option against gsr_l1_ssim_loss -- of the library given with --parent-library (the parent commit's
      build), or of this tree's when none is given: the no-option instantiation is expected to be the old kernels' work;
  (c) a stock-PyTorch fp32 evaluation of the formula of (a) with autograd (tests/torch_loss_ext.py with dtype=float32).

Every fused call goes straight to the C entry point with buffers allocated beforehand, so that the kernels are what is timed; wall
time between two events on the stream, the candidates alternated call by call in a rotating order, medians.  One JSON line, printed and appended to
profiles/loss_ext_bench.jsonl.

    python tools/loss_ext_bench.py --steps 50 --warmup 5 [--parent-library libgsr_hip_parent.so]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1980x1080,3840x2160")
    ap.add_argument("--parent-library", default=None, help="the parent commit's libgsr_hip.so: (b) runs its gsr_l1_ssim_loss")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "loss_ext_bench.jsonl"))
    args = ap.parse_args()

    import torch

    import fused_loss
    import torch_loss_ext as ref
    dev = torch.device("cuda:0")
    L = fused_loss._lib_ext()
    fused_loss._lib()
    old = L
    if args.parent_library:
        old = ctypes.CDLL(os.path.abspath(args.parent_library))
        old.gsr_loss_scratch_bytes.restype = ctypes.c_size_t
        old.gsr_loss_scratch_bytes.argtypes = [ctypes.c_int] * 3
        old.gsr_l1_ssim_loss.restype = ctypes.c_int
        old.gsr_l1_ssim_loss.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_float] + [ctypes.c_void_p] * 4
    stream = torch.cuda.current_stream(dev).cuda_stream

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    out = {"steps": args.steps, "warmup": args.warmup, "parent_library": bool(args.parent_library), "sizes": {}}
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        C = 3
        g = torch.Generator().manual_seed(1)
        rand = lambda *s: torch.rand(*s, generator=g).to(dev)
        gt = rand(C, H, W)
        x = (gt + 0.1 * torch.randn(C, H, W, generator=g).to(dev)).clamp(0, 1)
        mask, d, dp, dk = rand(H, W), rand(H, W), rand(H, W), rand(H, W)
        E = (torch.eye(3, 4) + 0.05 * torch.randn(3, 4, generator=g)).to(dev)
        vals = torch.empty(4, device=dev)
        gi, gE, gd = torch.empty(C, H, W, device=dev), torch.empty(3, 4, device=dev), torch.empty(H, W, device=dev)
        scratch = torch.empty(L.gsr_loss_ext_scratch_bytes(C, H, W), dtype=torch.uint8, device=dev)
        assert old.gsr_loss_scratch_bytes(C, H, W) <= scratch.numel()
        old_scratch = scratch   # one buffer for both: where the three maps lie relative to the images moves an HBM-bound kernel
        base = dict(C=C, H=H, W=W, lambda_dssim=0.2, img=x.data_ptr(), gt=gt.data_ptr(), vals=vals.data_ptr(), dL_dimg=gi.data_ptr(),
                    scratch=scratch.data_ptr(), stream=stream)
        a_all = fused_loss.LossExtArgs(**base, mask=mask.data_ptr(), exposure=E.data_ptr(), invdepth=d.data_ptr(),
                                       invdepth_prior=dp.data_ptr(), invdepth_mask=dk.data_ptr(), invdepth_weight=0.5,
                                       dL_dexposure=gE.data_ptr(), dL_dinvdepth=gd.data_ptr())
        a_none = fused_loss.LossExtArgs(**base)

        def run_ext(a):
            assert L.gsr_l1_ssim_loss_ext(ctypes.byref(a)) == 0, L.gsr_last_error()

        def run_old():
            assert old.gsr_l1_ssim_loss(C, H, W, x.data_ptr(), gt.data_ptr(), 0.2, vals.data_ptr(), gi.data_ptr(),
                                        old_scratch.data_ptr(), stream) == 0

        def run_stock():
            xs, Es, ds = (t.detach().clone().requires_grad_(True) for t in (x, E, d))
            ref.loss_terms(xs, gt, 0.2, mask, Es, ds, dp, dk, 0.5, dtype=torch.float32)[0].backward()

        runs = {"ext_all": lambda: run_ext(a_all), "ext_none": lambda: run_ext(a_none), "old": run_old, "stock": run_stock}
        ms = {k: [] for k in runs}
        names = list(runs)
        for it in range(args.warmup + args.steps):
            for k in names[it % len(names):] + names[:it % len(names)]:   # rotated: no candidate always runs behind the same one
                t = timed(runs[k])
                if it >= args.warmup:
                    ms[k].append(t)
        med = {k: statistics.median(v) for k, v in ms.items()}
        out["sizes"][size] = {"a_ext_all_options_ms": round(med["ext_all"], 4), "b_ext_no_option_ms": round(med["ext_none"], 4),
                              "b_l1_ssim_loss_ms": round(med["old"], 4), "c_stock_pytorch_ms": round(med["stock"], 4),
                              "b_ext_none_over_old": round(med["ext_none"] / med["old"], 3),
                              "a_ext_all_over_old": round(med["ext_all"] / med["old"], 3),
                              "c_stock_over_ext_all": round(med["stock"] / med["ext_all"], 2)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
