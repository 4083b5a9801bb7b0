"""The float64 dense autograd restatement of the depth-distortion map of include/gsr_distortion.h,
    Dist(p) = sum_{j<i} w_i w_j (v_i - v_j)^2 = A Q - D^2,   A = sum w, D = sum w (v - c), Q = sum w (v - c)^2,
with the image's own weights w = alpha T and the depth values v of the depth map (view-space z, or 1 / z).  TEST INFRASTRUCTURE, the
distortion counterpart of tests/torch_splat_feat.py, whose render() it calls with the two feature channels (v - c, (v - c)^2): same
conventions, same deliberate deviations, discrete decisions from the oracle state `o`.  v is computed in the same graph from means3D
and the view matrix, so dL/dv reaches means3D (and the camera tensors); gradients come from torch.autograd, so agreement with
csrc/distortion.hip checks its hand-written formulas rather than a copy of them.

The moment form is exact enough in float64 (and cancels in float32: with dtype=torch.float32 this function is the measure of what
an fp32 evaluation can reach -- centred at c = the mean v of the visible Gaussians by default, or raw with centre=0.0)."""
import torch

import torch_splat_cam
import torch_splat_feat


def depth_values(o, means3D, V, depth_mode, dtype=torch.float64):
    """v (P,) of the depth map's mode, in the graph of means3D and V ((4,4) or one copy per Gaussian); 0 for invisible Gaussians"""
    P = means3D.shape[0]
    Vp = torch_splat_cam._per_gaussian(V.to(dtype), P, (4, 4))
    hom = torch.cat([means3D.to(dtype), torch.ones(P, 1, dtype=dtype)], 1)
    tz = torch.einsum("pi,pij->pj", hom, Vp)[:, 2]
    vis = torch.from_numpy(o["radii"] > 0)
    tz = torch.where(vis, tz, torch.ones_like(tz))
    v = tz if depth_mode == "depth" else 1.0 / tz
    return torch.where(vis, v, torch.zeros_like(v)), vis


def render(o, means3D, scales, rotations, opacities, shs, depth_mode, V=None, PM=None, campos=None, dtype=torch.float64, centre=None,
           **kw):
    """-> (image (3,H,W), depth (H,W), alpha (H,W), distortion (H,W)).  depth_mode: "depth" / "invdepth"; centre: the constant c
    (default: the mean v of the visible Gaussians); **kw: the other keywords of torch_splat_cam.render (antialiasing, ...)."""
    Vt = torch.from_numpy(o["viewmatrix"]).reshape(4, 4) if V is None else V
    v, vis = depth_values(o, means3D, Vt, depth_mode, dtype)
    if centre is None:
        centre = float(v.detach()[vis].double().mean()) if bool(vis.any()) else 0.0
    u = torch.where(vis, v - centre, torch.zeros_like(v))
    img, D, A, m = torch_splat_feat.render(o, means3D, scales, rotations, opacities, shs, torch.stack([u, u * u], 1), V, PM, campos,
                                           dtype=dtype, depth_mode=depth_mode, **kw)
    return img, D, A, A * m[1] - m[0] * m[0]


def camera_terms(o, inputs, depth_mode, dL, **kw):
    """torch_splat_cam.camera_terms() for the loss sum(outputs * dL) over render()'s four outputs (dL: one tensor per output, None
    = the output is not in the loss) -> (total, abs_total, d32) over "V", "PM", "campos"."""
    P = inputs["means3D"].shape[0]
    out = {}
    for dt in (torch.float64, torch.float32):
        cam = {"V": inputs["V"].to(dt).expand(P, 4, 4).clone().requires_grad_(True),
               "PM": inputs["PM"].to(dt).expand(P, 4, 4).clone().requires_grad_(True),
               "campos": inputs["campos"].to(dt).expand(P, 3).clone().requires_grad_(True)}
        res = render(o, inputs["means3D"], inputs["scales"], inputs["rotations"], inputs["opacities"], inputs["shs"], depth_mode,
                     cam["V"], cam["PM"], cam["campos"], dtype=dt, **kw)
        loss = sum((r * d.to(dt).reshape(r.shape)).sum() for r, d in zip(res, dL) if d is not None)
        grads = torch.autograd.grad(loss, list(cam.values()), allow_unused=True)
        out[dt] = {k: (torch.zeros_like(cam[k]) if g is None else g).to(torch.float64) for k, g in zip(cam, grads)}
    total = {k: v.sum(0) for k, v in out[torch.float64].items()}
    abs_total = {k: v.abs().sum(0) for k, v in out[torch.float64].items()}
    d32 = {k: float((out[torch.float32][k].sum(0) - total[k]).abs().max()) for k in total}
    return total, abs_total, d32
