"""Fused training loss of the reference's loop (train.py:126-128, utils/loss_utils.py:16-63):

    Ll1 = l1_loss(image, gt_image)
    loss = (1.0 - opt.lambda_dssim) * Ll1 + opt.lambda_dssim * (1.0 - ssim(image, gt_image))
    loss.backward()

as ONE forward + ONE backward HIP kernel over the image (include/gsr.h gsr_l1_ssim_loss) instead of five
grouped conv2d, their autograd backward and the elementwise ops in between.  The backward's result is
the dL/dpix tensor the rasterizer's backward consumes.  HIP tensors only (no CPU fallback).
"""
import ctypes

import torch

from diff_gaussian_rasterization import _binding
from diff_gaussian_rasterization._binding import ptr


_lib, _run = _binding.declare("gsr.h", {
    "gsr_loss_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int] * 3),
    "gsr_l1_ssim_loss": (ctypes.c_int, [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_float] + [ctypes.c_void_p] * 4),
})


def l1_ssim_loss_and_grad(image, gt, lambda_dssim=0.2, want_grad=True):
    """-> (vals (3,) device tensor {loss, l1, ssim}, dloss/dimage (C,H,W) or None)"""
    if not image.is_cuda or not gt.is_cuda:
        raise RuntimeError("image and gt must be HIP (cuda) tensors; the fused loss has no CPU path")
    if image.shape != gt.shape or image.dim() != 3:
        raise RuntimeError(f"image and gt must both be (C,H,W); got {tuple(image.shape)} and {tuple(gt.shape)}")
    L = _lib()
    dev = image.device
    C, H, W = (int(v) for v in image.shape)
    img = image.detach().to(torch.float32).contiguous()
    g = gt.detach().to(device=dev, dtype=torch.float32).contiguous()
    with torch.cuda.device(dev):
        vals = torch.empty(3, dtype=torch.float32, device=dev)
        grad = torch.empty((C, H, W), dtype=torch.float32, device=dev) if want_grad else None
        scratch = torch.empty(L.gsr_loss_scratch_bytes(C, H, W), dtype=torch.uint8, device=dev)
        _run("gsr_l1_ssim_loss", C, H, W, img.data_ptr(), g.data_ptr(), float(lambda_dssim), vals.data_ptr(),
             grad.data_ptr() if want_grad else None, scratch.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        scratch.record_stream(torch.cuda.current_stream(dev))
    return vals, grad


class _L1SSIMLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, lambda_dssim):
        vals, grad = l1_ssim_loss_and_grad(image, gt, lambda_dssim, want_grad=image.requires_grad)
        ctx.save_for_backward(grad if grad is not None else torch.empty(0, device=image.device))
        loss, l1, s = vals[0], vals[1], vals[2]
        ctx.mark_non_differentiable(l1, s)   # the very objects that are returned: Ll1 and ssim are for logging only
        return loss, l1, s

    @staticmethod
    def backward(ctx, g_loss, g_l1, g_ssim):
        (grad,) = ctx.saved_tensors
        return (grad * g_loss if grad.numel() else None), None, None


def l1_ssim_loss(image, gt, lambda_dssim=0.2):
    """loss (scalar tensor, differentiable w.r.t. image) of train.py:127."""
    return _L1SSIMLoss.apply(image, gt, lambda_dssim)[0]


def l1_ssim_loss_terms(image, gt, lambda_dssim=0.2):
    """-> (loss, Ll1, ssim) as in train.py:126-127 (Ll1 and ssim are for logging, not differentiable)."""
    return _L1SSIMLoss.apply(image, gt, lambda_dssim)


# ---- the same loss with a pixel mask, a per-image exposure and an inverse-depth term (include/gsr_loss_ext.h) ----
#
#     x'_c = E[0][c] x_0 + E[1][c] x_1 + E[2][c] x_2 + E[c][3]        (exposure (3,4); x' = x without it)
#     x'' = m x',  y'' = m y                                          (mask (H,W) or (1,H,W) in [0,1]; both sides are masked)
#     Ll1depth = mean |(invdepth - invdepth_prior) invdepth_mask|
#     loss = (1 - lambda) mean|x'' - y''| + lambda (1 - SSIM(x'', y'')) + invdepth_weight Ll1depth
#
# still one forward kernel, one backward kernel and one fold; every option is optional, in every combination.

class LossExtArgs(ctypes.Structure):   # include/gsr_loss_ext.h gsr_loss_ext_args
    _fields_ = [("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("lambda_dssim", ctypes.c_float),
                ("img", ctypes.c_void_p), ("gt", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("exposure", ctypes.c_void_p),
                ("invdepth", ctypes.c_void_p), ("invdepth_prior", ctypes.c_void_p), ("invdepth_mask", ctypes.c_void_p),
                ("invdepth_weight", ctypes.c_float), ("vals", ctypes.c_void_p), ("dL_dimg", ctypes.c_void_p),
                ("dL_dexposure", ctypes.c_void_p), ("dL_dinvdepth", ctypes.c_void_p), ("scratch", ctypes.c_void_p),
                ("stream", ctypes.c_void_p)]


_WANT = ("image", "exposure", "invdepth")


_lib_ext = _binding.declare("gsr_loss_ext.h", {
    "gsr_loss_ext_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int] * 3),
    "gsr_l1_ssim_loss_ext": (ctypes.c_int, [ctypes.POINTER(LossExtArgs)]),
}, {"gsr_loss_ext_args": LossExtArgs})[0]


def _check_training_loss(image, gt, mask, exposure, invdepth, invdepth_prior, invdepth_mask, invdepth_weight, want):
    """Every refusal of the extended loss, before the kernel library is touched.  -> (C, H, W)"""
    if not torch.is_tensor(image) or not torch.is_tensor(gt):
        raise ValueError("image and gt must be tensors")
    if image.dim() != 3 or image.shape != gt.shape:
        raise RuntimeError(f"image and gt must both be (C,H,W); got {tuple(image.shape)} and {tuple(gt.shape)}")
    C, H, W = (int(v) for v in image.shape)
    if C <= 0 or H <= 0 or W <= 0:
        raise RuntimeError(f"image must not be empty; got {tuple(image.shape)}")
    if image.dtype != torch.float32 or gt.dtype != torch.float32:
        raise RuntimeError(f"image and gt must be float32; got {image.dtype} and {gt.dtype}")

    def plane(name, t, dtypes=(torch.float32,)):
        if not torch.is_tensor(t):
            raise ValueError(f"{name} must be a tensor or None")
        if tuple(t.shape) not in ((H, W), (1, H, W)):
            raise RuntimeError(f"{name} must be (H,W) or (1,H,W) = ({H},{W}); got {tuple(t.shape)}")
        if t.dtype not in dtypes:
            raise RuntimeError(f"{name} must be {' or '.join(str(d) for d in dtypes)}; got {t.dtype}")
        if t.device != image.device:
            raise RuntimeError(f"{name} must be on the image's device {image.device}; got {t.device}")

    if mask is not None:
        plane("mask", mask, (torch.float32, torch.bool))
    if exposure is not None:
        if not torch.is_tensor(exposure):
            raise ValueError("exposure must be a tensor or None")
        if C != 3:
            raise ValueError(f"exposure needs a 3-channel image; got C = {C}")
        if tuple(exposure.shape) != (3, 4) or exposure.dtype != torch.float32 or exposure.device != image.device:
            raise RuntimeError(f"exposure must be a float32 (3,4) tensor on {image.device}; got {tuple(exposure.shape)} {exposure.dtype} "
                               f"on {exposure.device}")
    if (invdepth is None) != (invdepth_prior is None):
        raise ValueError("invdepth and invdepth_prior go together: give both or neither")
    if invdepth is None and invdepth_mask is not None:
        raise ValueError("invdepth_mask without invdepth and invdepth_prior")
    if invdepth is not None:
        plane("invdepth", invdepth)
        plane("invdepth_prior", invdepth_prior)
        if invdepth_mask is not None:
            plane("invdepth_mask", invdepth_mask, (torch.float32, torch.bool))
    w = float(invdepth_weight)
    if not (w >= 0.0) or w == float("inf"):
        raise ValueError(f"invdepth_weight must be finite and >= 0; got {invdepth_weight}")
    want = tuple(want)
    for k in want:
        if k not in _WANT:
            raise ValueError(f"want: unknown gradient {k!r}; the choices are {_WANT}")
    if not image.is_cuda or gt.device != image.device:
        raise RuntimeError("image and gt must be HIP (cuda) tensors on one device; the fused loss has no CPU path")
    return C, H, W


def training_loss_and_grads(image, gt, lambda_dssim=0.2, *, mask=None, exposure=None, invdepth=None, invdepth_prior=None,
                            invdepth_mask=None, invdepth_weight=0.0, want=_WANT):
    """-> (vals (4,) device tensor {loss, l1, ssim, depth_l1}, {"image": dloss/dimage (C,H,W), "exposure": dloss/dexposure (3,4),
    "invdepth": dloss/dinvdepth in invdepth's shape}), raw and without autograd.  The dictionary holds the gradients named in `want`
    whose input was given."""
    C, H, W = _check_training_loss(image, gt, mask, exposure, invdepth, invdepth_prior, invdepth_mask, invdepth_weight, want)
    L = _lib_ext()
    dev = image.device
    f32 = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()
    img, g, m, E, d, dp, dk = (f32(t) for t in (image, gt, mask, exposure, invdepth, invdepth_prior, invdepth_mask))
    with torch.cuda.device(dev):
        vals = torch.empty(4, dtype=torch.float32, device=dev)
        grads = {}
        if "image" in want:
            grads["image"] = torch.empty((C, H, W), dtype=torch.float32, device=dev)
        if "exposure" in want and E is not None:
            grads["exposure"] = torch.empty((3, 4), dtype=torch.float32, device=dev)
        if "invdepth" in want and d is not None:
            grads["invdepth"] = torch.empty(tuple(invdepth.shape), dtype=torch.float32, device=dev)
        scratch = torch.empty(L.gsr_loss_ext_scratch_bytes(C, H, W), dtype=torch.uint8, device=dev)
        a = LossExtArgs(C=C, H=H, W=W, lambda_dssim=float(lambda_dssim), img=ptr(img), gt=ptr(g), mask=ptr(m), exposure=ptr(E),
                        invdepth=ptr(d), invdepth_prior=ptr(dp), invdepth_mask=ptr(dk), invdepth_weight=float(invdepth_weight),
                        vals=ptr(vals), dL_dimg=ptr(grads.get("image")), dL_dexposure=ptr(grads.get("exposure")),
                        dL_dinvdepth=ptr(grads.get("invdepth")), scratch=ptr(scratch), stream=torch.cuda.current_stream(dev).cuda_stream)
        _run("gsr_l1_ssim_loss_ext", ctypes.byref(a))
        scratch.record_stream(torch.cuda.current_stream(dev))
    return vals, grads


class _TrainingLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, exposure, invdepth, gt, lambda_dssim, mask, invdepth_prior, invdepth_mask, invdepth_weight):
        needs = ctx.needs_input_grad[:3]   # gradients are computed for the inputs that require them, and for no other
        want = tuple(name for name, need in zip(_WANT, needs) if need)
        vals, grads = training_loss_and_grads(image, gt, lambda_dssim, mask=mask, exposure=exposure, invdepth=invdepth,
                                              invdepth_prior=invdepth_prior, invdepth_mask=invdepth_mask,
                                              invdepth_weight=invdepth_weight, want=want)
        ctx.names = tuple(name for name in _WANT if name in grads)
        ctx.save_for_backward(*(grads[name] for name in ctx.names))
        loss, l1, s, ld = vals[0], vals[1], vals[2], vals[3]
        ctx.mark_non_differentiable(l1, s, ld)   # the very objects that are returned: they are for logging only
        return loss, l1, s, ld

    @staticmethod
    def backward(ctx, g_loss, g_l1, g_ssim, g_ld):
        grads = dict(zip(ctx.names, ctx.saved_tensors))
        out = tuple(grads[name] * g_loss if name in grads else None for name in _WANT)
        return out + (None,) * 6


def training_loss_terms(image, gt, lambda_dssim=0.2, *, mask=None, exposure=None, invdepth=None, invdepth_prior=None,
                        invdepth_mask=None, invdepth_weight=0.0, want=_WANT):
    """-> (loss, Ll1, ssim, Ll1depth): loss is differentiable w.r.t. image, exposure and invdepth (those of them in `want` that
    require a gradient); the other three are for logging."""
    _check_training_loss(image, gt, mask, exposure, invdepth, invdepth_prior, invdepth_mask, invdepth_weight, want)
    keep = lambda name, t: t if (t is None or name in want) else t.detach()
    return _TrainingLoss.apply(keep("image", image), keep("exposure", exposure), keep("invdepth", invdepth), gt, float(lambda_dssim),
                               mask, invdepth_prior, invdepth_mask, float(invdepth_weight))


def training_loss(image, gt, lambda_dssim=0.2, **options):
    """loss (scalar tensor) of training_loss_terms: the options are its keywords."""
    return training_loss_terms(image, gt, lambda_dssim, **options)[0]
