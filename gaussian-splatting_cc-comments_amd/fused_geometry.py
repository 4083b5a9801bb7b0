"""Fused normal-consistency term of surface-reconstruction training on splats (2DGS, PGSR, RaDe-GS, GOF, Gaussian surfels), beside
fused_loss.py (include/gsr_normals.h is the contract):

    n        = gaussian_normals(scales, rotations, means3D, viewmatrix)          # (P, 3), one kernel; backward: one kernel
    out      = render(..., depth_alpha="depth", normals=True)                    # blends n with the colour pass's weights
    loss_n   = normal_consistency_loss(out["normal"], out["depth"] / out["alpha"], out["alpha"], tanfovx, tanfovy)
    normals  = depth_normals(depth, tanfovx, tanfovy)                            # (3, H, W), for inspection or other losses

instead of about forty stock-PyTorch passes with their autograd backward.  The loss and both of its gradients come from ONE kernel
over the image plus a fixed-order fold.  Which depth goes into the loss (depth / alpha, the median depth, a mix) is the caller's
choice, made in torch.  HIP float32 tensors only: there is no CPU path.
"""
import torch

from diff_gaussian_rasterization import _C


def _hip_f32(named):
    """named: (tensor, name, allowed shapes) triples -> their contiguous, detached forms, all float32 HIP tensors on one device.
    Anything else is refused before the library is touched: TypeError for a non-tensor, RuntimeError for a wrong dtype or shape (checked
    for every tensor first), then for a CPU tensor or a second device."""
    for t, name, shapes in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a float32 tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be float32 (got {t.dtype})")
        if tuple(t.shape) not in shapes:
            raise RuntimeError(f"{name} must have shape {' or '.join(str(s) for s in shapes)} (got {tuple(t.shape)})")
    device = named[0][0].device
    for t, name, _ in named:
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a HIP (cuda) tensor (got {t.device}); the fused geometry kernels have no CPU path")
        if t.device != device:
            raise RuntimeError(f"{name} must be on {device}, the device of {named[0][1]} (got {t.device})")
    return [t.detach().contiguous() for t, _, _ in named]


def _tan(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{name} must be a number, got {type(v).__name__}")
    return float(v)


def _gaussian_inputs(scales, rotations, means3D, viewmatrix, space):
    if not isinstance(space, str) or space not in _C.NORMAL_SPACES:
        raise ValueError(f"space must be one of {sorted(_C.NORMAL_SPACES)}, got {space!r}")
    if not isinstance(rotations, torch.Tensor):
        raise TypeError(f"rotations must be a float32 tensor, got {type(rotations).__name__}")
    P = int(rotations.size(0)) if rotations.dim() else -1
    q, s, m, v = _hip_f32(((rotations, "rotations", ((P, 4),)), (scales, "scales", ((P, 3),)), (means3D, "means3D", ((P, 3),)),
                           (viewmatrix, "viewmatrix", ((4, 4), (16,)))))
    return s, q, m, v, _C.NORMAL_SPACES[space]


class _GaussianNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scales, rotations, means3D, viewmatrix, space):
        s, q, m, v, sp = _gaussian_inputs(scales, rotations, means3D, viewmatrix, space)
        dev, P = q.device, int(q.size(0))
        with torch.cuda.device(dev):
            out = torch.empty((P, 3), dtype=torch.float32, device=dev)
            _C._check(_C.lib().gsr_gaussian_normals(P, _C._ptr(s), _C._ptr(q), _C._ptr(m), _C._ptr(v), sp, _C._ptr(out), _C._stream(dev)))
        ctx.save_for_backward(s, q, m, v)
        ctx.space = sp
        return out

    @staticmethod
    def backward(ctx, g):
        s, q, m, v = ctx.saved_tensors
        dev, P = q.device, int(q.size(0))
        g = _C._dev_f32(g, dev, "dL_dnormals")
        with torch.cuda.device(dev):
            dq = torch.empty((P, 4), dtype=torch.float32, device=dev)
            _C._check(_C.lib().gsr_gaussian_normals_backward(P, _C._ptr(s), _C._ptr(q), _C._ptr(m), _C._ptr(v), ctx.space, _C._ptr(g),
                                                             _C._ptr(dq), _C._stream(dev)))
        return None, dq, None, None, None


def gaussian_normals(scales, rotations, means3D, viewmatrix, space="view"):
    """-> (P, 3): per Gaussian the axis of its smallest scale (the first on an exact tie; log-scales choose the same axis), rotated by
    the normalised quaternion, flipped to face the camera, in view space (space="view": rotated by viewmatrix[:3, :3] as the
    rasterizer reads it) or world space (space="world").  Differentiable w.r.t. `rotations` (through the normalisation; the axis
    choice and the sign are constants); scales, means3D and viewmatrix receive no gradient.  Every row is written: nothing is culled."""
    return _GaussianNormals.apply(scales, rotations, means3D, viewmatrix, space)


def _depth_size(depth):
    if not isinstance(depth, torch.Tensor):
        raise TypeError(f"depth must be a float32 tensor, got {type(depth).__name__}")
    if depth.dim() not in (2, 3) or (depth.dim() == 3 and depth.size(0) != 1) or depth.numel() == 0:
        raise RuntimeError(f"depth must have shape (H, W) or (1, H, W) (got {tuple(depth.shape)})")
    return int(depth.size(-2)), int(depth.size(-1))


class _DepthNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, tanfovx, tanfovy):
        tx, ty = _tan(tanfovx, "tanfovx"), _tan(tanfovy, "tanfovy")
        H, W = _depth_size(depth)
        (d,) = _hip_f32(((depth, "depth", ((H, W), (1, H, W))),))
        dev = d.device
        with torch.cuda.device(dev):
            out = torch.empty((3, H, W), dtype=torch.float32, device=dev)
            _C._check(_C.lib().gsr_depth_normals(W, H, _C._ptr(d), tx, ty, _C._ptr(out), _C._stream(dev)))
        ctx.save_for_backward(d)
        ctx.tan, ctx.shape = (tx, ty), tuple(depth.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        dev, H, W = d.device, int(d.size(-2)), int(d.size(-1))
        g = _C._dev_f32(g, dev, "dL_dnormals")
        with torch.cuda.device(dev):
            dd = torch.empty(ctx.shape, dtype=torch.float32, device=dev)
            _C._check(_C.lib().gsr_depth_normals_backward(W, H, _C._ptr(d), *ctx.tan, _C._ptr(g), _C._ptr(dd), _C._stream(dev)))
        return dd, None, None


def depth_normals(depth, tanfovx, tanfovy):
    """-> (3, H, W): view-space normals of the surface of `depth` ((H, W) or (1, H, W), view-space z), 2DGS's depth_to_normal: the
    normalised cross product of the central differences of the unprojected points.  Zeros at border pixels and wherever one of the
    four axis neighbours' depths is not finite and > 0.  Differentiable w.r.t. `depth`."""
    return _DepthNormals.apply(depth, tanfovx, tanfovy)


def normal_consistency_loss_and_grads(normal_map, depth, alpha, tanfovx, tanfovy, want_normal_grad=True, want_depth_grad=True):
    """-> (vals (1,) device tensor {loss}, dloss/dnormal_map (3, H, W) or None, dloss/ddepth in depth's shape or None), one launch."""
    tx, ty = _tan(tanfovx, "tanfovx"), _tan(tanfovy, "tanfovy")
    H, W = _depth_size(depth)
    d, n, a = (_hip_f32(((depth, "depth", ((H, W), (1, H, W))), (normal_map, "normal_map", ((3, H, W),))) +
                        (() if alpha is None else ((alpha, "alpha", ((H, W), (1, H, W))),))) + [None])[:3]
    dev = d.device
    L = _C.lib()
    with torch.cuda.device(dev):
        f32 = dict(dtype=torch.float32, device=dev)
        vals = torch.empty(1, **f32)
        dn = torch.empty((3, H, W), **f32) if want_normal_grad else None
        dd = torch.empty(tuple(depth.shape), **f32) if want_depth_grad else None
        scratch = torch.empty(L.gsr_normals_scratch_bytes(W, H), dtype=torch.uint8, device=dev)
        _C._check(L.gsr_normal_consistency_loss(W, H, _C._ptr(n), _C._ptr(d), _C._ptr(a), tx, ty, _C._ptr(vals), _C._ptr(dn), _C._ptr(dd),
                                                _C._ptr(scratch), _C._stream(dev)))
        _C.release_scratch(scratch, dev)
    return vals, dn, dd


class _NormalConsistencyLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normal_map, depth, alpha, tanfovx, tanfovy):
        vals, dn, dd = normal_consistency_loss_and_grads(normal_map, depth, alpha, tanfovx, tanfovy, ctx.needs_input_grad[0],
                                                         ctx.needs_input_grad[1])
        empty = torch.empty(0, device=vals.device)
        ctx.save_for_backward(dn if dn is not None else empty, dd if dd is not None else empty)
        return vals[0]

    @staticmethod
    def backward(ctx, g):
        dn, dd = ctx.saved_tensors
        return (dn * g if ctx.needs_input_grad[0] and dn.numel() else None), (dd * g if ctx.needs_input_grad[1] and dd.numel() else None), \
            None, None, None


def normal_consistency_loss(normal_map, depth, alpha, tanfovx, tanfovy):
    """loss (scalar tensor) = mean over all H W pixels of 1 - alpha <normal_map, depth_normals(depth)>: 2DGS's normal_error.mean() with
    the depth normals multiplied by the detached alpha ((H, W) or (1, H, W); None = 1).  Differentiable w.r.t. normal_map (3, H, W) and
    depth ((H, W) or (1, H, W)); alpha receives no gradient.  Value and gradients come from the one forward call."""
    return _NormalConsistencyLoss.apply(normal_map, depth, alpha, tanfovx, tanfovy)
