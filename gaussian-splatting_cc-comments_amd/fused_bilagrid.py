"""Per-image bilateral grid of affine colour transforms ("Bilateral Guided Radiance Field Processing"; gsplat's --use_bilateral_grid,
lib_bilagrid `slice` and `total_variation_loss`) as fused HIP kernels (include/gsr_bilagrid.h): the spatially varying form of
fused_loss's 3x4 exposure.  Every pixel takes its own 3x4 transform from a small 3-D grid -- its position gives two coordinates, its
own luma the third:

    gx = (x + 0.5) / W * (GW - 1),  gy = (y + 0.5) / H * (GH - 1),  gz = clamp((0.299 r + 0.587 g + 0.114 b) * (L - 1), 0, L - 1)
    A = trilinear interpolation of the grid's twelve channels at (gz, gy, gx),   out_c = A[c][0] r + A[c][1] g + A[c][2] b + A[c][3]

which stock PyTorch writes as a meshgrid, a matmul, a 5-D grid_sample (align_corners=True, padding_mode="border"), a permute and a
batched matmul.  One kernel forward, a kernel per gradient backward, no atomics: every output is bitwise reproducible.

    bg = BilateralGrid(num_images)
    loss = fused_loss.training_loss(bilateral_grid_slice(bg.grids[i], image), gt) + 10 * bg.tv_loss()

HIP tensors only (no CPU fallback).
"""
import ctypes

import torch

from diff_gaussian_rasterization import _binding
from diff_gaussian_rasterization._binding import ptr


class BilagridArgs(ctypes.Structure):   # include/gsr_bilagrid.h gsr_bilagrid_args
    _fields_ = [("H", ctypes.c_int), ("W", ctypes.c_int), ("L", ctypes.c_int), ("GH", ctypes.c_int), ("GW", ctypes.c_int),
                ("grid", ctypes.c_void_p), ("img", ctypes.c_void_p), ("out", ctypes.c_void_p), ("dL_dout", ctypes.c_void_p),
                ("dL_dgrid", ctypes.c_void_p), ("dL_dimg", ctypes.c_void_p), ("scratch", ctypes.c_void_p), ("stream", ctypes.c_void_p)]


_WANT = ("grid", "image")
_lib, _run = _binding.declare("gsr_bilagrid.h", {
    "gsr_bilagrid_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int] * 5),
    "gsr_bilagrid_slice": (ctypes.c_int, [ctypes.POINTER(BilagridArgs)]),
    "gsr_bilagrid_slice_backward": (ctypes.c_int, [ctypes.POINTER(BilagridArgs)]),
    "gsr_bilagrid_tv_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int] * 4),
    "gsr_bilagrid_tv": (ctypes.c_int, [ctypes.c_int] * 4 + [ctypes.c_void_p] * 5),
}, {"gsr_bilagrid_args": BilagridArgs})


def _check_grid_shape(name, shape):
    if len(shape) != 4 or shape[0] != 12:
        raise RuntimeError(f"{name} must be (12, L, GH, GW); got {tuple(shape)}")
    if min(shape[1:]) < 2:
        raise RuntimeError(f"{name}: every grid axis (L, GH, GW) must be at least 2; got {tuple(shape)}")


def _check_slice(grid, image, grad_out=None, want=_WANT):
    """Every refusal of the slice, before the kernel library is touched.  -> (H, W, L, GH, GW)"""
    if not torch.is_tensor(grid) or not torch.is_tensor(image) or not (grad_out is None or torch.is_tensor(grad_out)):
        raise TypeError("grid, image and grad_out must be tensors")
    if image.dim() != 3 or image.shape[0] != 3 or image.shape[1] < 1 or image.shape[2] < 1:
        raise RuntimeError(f"image must be (3, H, W); got {tuple(image.shape)}")
    _check_grid_shape("grid", grid.shape)
    if grad_out is not None and grad_out.shape != image.shape:
        raise RuntimeError(f"grad_out must have the image's shape {tuple(image.shape)}; got {tuple(grad_out.shape)}")
    for name, t in (("grid", grid), ("image", image), ("grad_out", grad_out)):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be float32; got {t.dtype}")
    want = tuple(want)
    for k in want:
        if k not in _WANT:
            raise ValueError(f"want: unknown gradient {k!r}; the choices are {_WANT}")
    if grad_out is not None and not want:
        raise ValueError("want: name at least one gradient")
    if not image.is_cuda or grid.device != image.device or (grad_out is not None and grad_out.device != image.device):
        raise RuntimeError("grid, image and grad_out must be HIP (cuda) tensors on one device; the bilateral grid has no CPU path")
    return tuple(int(v) for v in image.shape[1:]) + tuple(int(v) for v in grid.shape[1:])


def _slice_raw(grid, image):
    H, W, L, GH, GW = _check_slice(grid, image)
    dev = image.device
    g, x = grid.detach().contiguous(), image.detach().contiguous()
    with torch.cuda.device(dev):
        out = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        a = BilagridArgs(H=H, W=W, L=L, GH=GH, GW=GW, grid=g.data_ptr(), img=x.data_ptr(), out=out.data_ptr(),
                         stream=torch.cuda.current_stream(dev).cuda_stream)
        _run("gsr_bilagrid_slice", ctypes.byref(a))
    return out


def slice_and_grads(grid, image, grad_out, want=_WANT):
    """-> (out (3,H,W), {"grid": dL/dgrid (12,L,GH,GW), "image": dL/dimage (3,H,W)}) for grad_out = dL/dout, raw and without autograd.
    The dictionary holds the gradients named in `want`."""
    H, W, L, GH, GW = _check_slice(grid, image, grad_out, want)
    out = _slice_raw(grid, image)
    return out, _slice_backward_raw(grid, image, grad_out, tuple(want))


def _slice_backward_raw(grid, image, grad_out, want):
    H, W, L, GH, GW = _check_slice(grid, image, grad_out, want)
    lib = _lib()
    dev = image.device
    g, x, go = grid.detach().contiguous(), image.detach().contiguous(), grad_out.detach().contiguous()
    with torch.cuda.device(dev):
        grads = {}
        if "grid" in want:
            grads["grid"] = torch.empty((12, L, GH, GW), dtype=torch.float32, device=dev)
        if "image" in want:
            grads["image"] = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        scratch = torch.empty(lib.gsr_bilagrid_scratch_bytes(H, W, L, GH, GW), dtype=torch.uint8, device=dev)
        a = BilagridArgs(H=H, W=W, L=L, GH=GH, GW=GW, grid=g.data_ptr(), img=x.data_ptr(), dL_dout=go.data_ptr(),
                         dL_dgrid=ptr(grads.get("grid")), dL_dimg=ptr(grads.get("image")), scratch=scratch.data_ptr(),
                         stream=torch.cuda.current_stream(dev).cuda_stream)
        _run("gsr_bilagrid_slice_backward", ctypes.byref(a))
        scratch.record_stream(torch.cuda.current_stream(dev))
    return grads


class _Slice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, image):
        ctx.save_for_backward(grid, image)
        return _slice_raw(grid, image)

    @staticmethod
    def backward(ctx, grad_out):
        grid, image = ctx.saved_tensors
        want = tuple(name for name, need in zip(_WANT, ctx.needs_input_grad) if need)   # and no other gradient is computed
        if not want:
            return None, None
        grads = _slice_backward_raw(grid, image, grad_out, want)
        return grads.get("grid"), grads.get("image")


def bilateral_grid_slice(grid, image):
    """image (3,H,W) through grid (12,L,GH,GW) -> (3,H,W); differentiable w.r.t. both.  A non-contiguous input is made contiguous;
    grids[idx] of a contiguous (N,12,L,GH,GW) parameter is used where it lies."""
    _check_slice(grid, image)
    return _Slice.apply(grid, image)


def _check_tv(grids):
    if not torch.is_tensor(grids):
        raise TypeError("grids must be a tensor")
    if grids.dim() not in (4, 5):
        raise RuntimeError(f"grids must be (N, 12, L, GH, GW) or (12, L, GH, GW); got {tuple(grids.shape)}")
    shape = tuple(int(v) for v in grids.shape)
    if len(shape) == 5 and shape[0] < 1:
        raise RuntimeError(f"grids must hold at least one grid; got {shape}")
    _check_grid_shape("grids", shape[-4:])
    if grids.dtype != torch.float32:
        raise RuntimeError(f"grids must be float32; got {grids.dtype}")
    if not grids.is_cuda:
        raise RuntimeError("grids must be a HIP (cuda) tensor; the bilateral grid has no CPU path")
    return (shape[0] if len(shape) == 5 else 1,) + shape[-3:]


def tv_and_grad(grids, want_grad=True):
    """-> (tv (1,) device tensor, d tv / d grids in grids' shape or None), raw and without autograd."""
    N, L, GH, GW = _check_tv(grids)
    lib = _lib()
    dev = grids.device
    g = grids.detach().contiguous()
    with torch.cuda.device(dev):
        val = torch.empty(1, dtype=torch.float32, device=dev)
        grad = torch.empty(tuple(grids.shape), dtype=torch.float32, device=dev) if want_grad else None
        scratch = torch.empty(lib.gsr_bilagrid_tv_scratch_bytes(N, L, GH, GW), dtype=torch.uint8, device=dev)
        _run("gsr_bilagrid_tv", N, L, GH, GW, g.data_ptr(), val.data_ptr(), grad.data_ptr() if want_grad else None, scratch.data_ptr(),
             torch.cuda.current_stream(dev).cuda_stream)
        scratch.record_stream(torch.cuda.current_stream(dev))
    return val, grad


class _TotalVariation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        val, grad = tv_and_grad(grids, want_grad=ctx.needs_input_grad[0])   # the gradient is formed here, in the same pass
        ctx.save_for_backward(grad if grad is not None else torch.empty(0, device=grids.device))
        return val[0]

    @staticmethod
    def backward(ctx, g_val):
        (grad,) = ctx.saved_tensors
        return grad * g_val if grad.numel() else None


def total_variation_loss(grids):
    """gsplat's total_variation_loss of (N,12,L,GH,GW) or (12,L,GH,GW) grids: a scalar tensor, differentiable."""
    _check_tv(grids)
    return _TotalVariation.apply(grids)


class BilateralGrid(torch.nn.Module):
    """`num` per-image grids: one parameter `grids` (num, 12, grid_W, grid_Y, grid_X) -- grid_W is the luma axis -- initialised to
    the identity transform at every node.  One FusedAdam group: FusedAdam([{"params": [bg.grids], "lr": 2e-3}])."""

    def __init__(self, num, grid_X=16, grid_Y=16, grid_W=8):
        super().__init__()
        num, grid_X, grid_Y, grid_W = int(num), int(grid_X), int(grid_Y), int(grid_W)
        if num < 1 or min(grid_X, grid_Y, grid_W) < 2:
            raise ValueError(f"BilateralGrid needs num >= 1 and every grid axis >= 2; got {num}, {grid_X}, {grid_Y}, {grid_W}")
        eye = torch.eye(3, 4, dtype=torch.float32).reshape(1, 12, 1, 1, 1)
        self.grids = torch.nn.Parameter(eye.repeat(num, 1, grid_W, grid_Y, grid_X))

    def forward(self, image, idx):
        """image (3,H,W) through the grid of image `idx`"""
        return bilateral_grid_slice(self.grids[int(idx)], image)

    def tv_loss(self):
        return total_variation_loss(self.grids)
