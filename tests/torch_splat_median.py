"""The float64 dense restatement of the median-depth map and the per-pixel index maps of include/gsr_median.h.  TEST INFRASTRUCTURE,
built on tests/torch_splat_feat.py's render(): one-hot feature channels give every weight w_i(p) = alpha_i T_i of the image's own
blend (same conventions, same deliberate deviations, discrete decisions from the oracle state `o`), the list order is the global
(depth, index) order of tests/torch_splat.py restricted to the visible Gaussians, and T_i = 1 - sum_{j<i} w_j.  From these, per pixel:
    median   = the last blended Gaussian with T_i > 0.5          dominant = the first blended Gaussian with the largest w_i
The median depth is a GATHER of torch_splat_dist.depth_values() at the median index, so autograd yields exactly the gradient the
header defines -- dL/dv_i = the sum of g over the pixels whose median is i, nothing through alpha or T -- by a route that shares no
formula with csrc/median.hip.

The dense blend costs (P / 3) passes of P x H x W pairs: for small scenes only."""
import numpy as np
import torch

import torch_splat_dist
import torch_splat_feat

T_MARGIN = 1e-4     # a blended T_i this close to 0.5 makes the median's choice a matter of rounding
W_MARGIN = 1e-5     # ... and so do two largest weights this close to each other (relative)


def list_order(o):
    """Gaussian ids in the order every tile list holds them: (depth, index), visible ones only (tests/torch_splat.py:96)"""
    P = o["radii"].shape[0]
    order = np.lexsort((np.arange(P), o["depths"]))
    return torch.from_numpy(order[o["radii"][order] > 0].astype(np.int64))


def weights(o, means3D, scales, rotations, opacities, shs, dtype=torch.float64, **kw):
    """-> w (P, H * W), detached: the blend weight of every (Gaussian, pixel) pair, 0 where the pair did not blend"""
    P = means3D.shape[0]
    with torch.no_grad():
        fmap = torch_splat_feat.render(o, means3D.detach(), scales.detach(), rotations.detach(), opacities.detach(), shs.detach(),
                                       torch.eye(P, dtype=dtype), dtype=dtype, **kw)[-1]
    return fmap.reshape(P, -1)


def choose(o, w):
    """-> dict of (H, W) tensors from the weights w (P, N): median_index, dominant_index (int64, -1 where nothing blends),
    dominant_weight, hit (bool), crossed (bool: T fell to 0.5 or below behind the median, i.e. the median is not the last hit),
    ambiguous (bool: a blended T_i within T_MARGIN of 0.5, the two largest weights within W_MARGIN relative, or a pixel the oracle
    calls fragile)"""
    H, W = o["H"], o["W"]
    order = list_order(o)
    N = w.shape[1]
    if order.numel() == 0:
        none = torch.full((H, W), -1, dtype=torch.int64)
        f = torch.zeros(H, W, dtype=torch.bool)
        return dict(median_index=none, dominant_index=none.clone(), dominant_weight=torch.zeros(H, W, dtype=w.dtype), hit=f, crossed=f,
                    ambiguous=torch.from_numpy((o["fragile"] != 0).reshape(H, W)))
    wo = w[order]                                   # (n, N) in list order
    blended = wo > 0
    Tin = 1.0 - (torch.cumsum(wo, 0) - wo)          # T in front of each Gaussian
    rank = torch.arange(1, wo.shape[0] + 1)[:, None]
    hit = blended.any(0)
    med = ((blended & (Tin > 0.5)).to(torch.int64) * rank).max(0).values - 1      # the last one; the first blended has T = 1 exactly
    last = (blended.to(torch.int64) * rank).max(0).values - 1
    dom = torch.argmax(wo, 0)                       # the first of the maximal values
    top = torch.topk(wo, min(2, wo.shape[0]), 0).values
    tie = (top[0] - top[-1] <= W_MARGIN * top[0]) & hit if wo.shape[0] > 1 else torch.zeros(N, dtype=torch.bool)
    near = (blended & ((Tin - 0.5).abs() <= T_MARGIN)).any(0)
    ambiguous = near | tie | torch.from_numpy((o["fragile"] != 0).reshape(-1))
    none = torch.full((N,), -1, dtype=torch.int64)
    return dict(median_index=torch.where(hit, order[med.clamp_min(0)], none).reshape(H, W),
                dominant_index=torch.where(hit, order[dom], none).reshape(H, W),
                dominant_weight=torch.where(hit, wo.max(0).values, torch.zeros_like(top[0])).reshape(H, W),
                hit=hit.reshape(H, W), crossed=(hit & (med != last)).reshape(H, W), ambiguous=ambiguous.reshape(H, W))


def median_depth(o, means3D, median_index, depth_mode, V=None, dtype=torch.float64):
    """-> (H, W): v of the pixel's median Gaussian in the graph of means3D (and V), 0 where median_index is -1"""
    Vt = torch.from_numpy(o["viewmatrix"]).reshape(4, 4) if V is None else V
    v, _ = torch_splat_dist.depth_values(o, means3D, Vt, depth_mode, dtype)
    return torch.where(median_index >= 0, v[median_index.clamp_min(0)], torch.zeros((), dtype=dtype))


def render(o, means3D, scales, rotations, opacities, shs, depth_mode, V=None, PM=None, campos=None, dtype=torch.float64, **kw):
    """-> (image (3,H,W), depth (H,W), alpha (H,W), median_depth (H,W), maps: the dict of choose()).  The first three are
    torch_splat_feat.render()'s; **kw: the other keywords of torch_splat_cam.render (antialiasing, ...)."""
    P = means3D.shape[0]
    maps = choose(o, weights(o, means3D, scales, rotations, opacities, shs, dtype, **kw))
    img, D, A, _ = torch_splat_feat.render(o, means3D, scales, rotations, opacities, shs, torch.zeros(P, 1, dtype=dtype), V, PM, campos,
                                           dtype=dtype, depth_mode=depth_mode, **kw)
    return img, D, A, median_depth(o, means3D, maps["median_index"], depth_mode, V, dtype), maps
