"""Reference of the extended fused loss (include/gsr_loss_ext.h) in plain torch with autograd, written from its definition:

    x'_c = E[0][c] x_0 + E[1][c] x_1 + E[2][c] x_2 + E[c][3]           (x' = x without exposure)
    x''  = m x',  y'' = m y                                            (m = 1 without a mask)
    L1   = mean |x'' - y''|
    SSIM = 11x11 window, sigma 1.5, taps built in float32, zero padding of x'' and y'', C1 = 1e-4, C2 = 9e-4, mean over C H W
    Ld   = mean |(d - d*) k|                                           (k = 1 without a depth mask; 0 without a depth term)
    loss = (1 - lambda) L1 + lambda (1 - SSIM) + w Ld

dtype=torch.float64 is the truth, the same code with dtype=torch.float32 the measure of what fp32 arithmetic costs.
"""
import math

import numpy as np
import torch


def taps(dtype, device):
    """the window's taps as the kernels hold them: float32 exp, divided by their float32 sum"""
    raw = [np.float32(math.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2))) for k in range(11)]
    total = np.float32(0.0)
    for r in raw:   # summed in order, in float32
        total = np.float32(total + r)
    return torch.tensor([float(np.float32(r / total)) for r in raw], dtype=torch.float64).to(device=device, dtype=dtype)


def loss_terms(image, gt, lambda_dssim=0.2, mask=None, exposure=None, invdepth=None, invdepth_prior=None, invdepth_mask=None,
               invdepth_weight=0.0, dtype=torch.float64):
    """-> (loss, l1, ssim, depth_l1), differentiable w.r.t. whichever of image, exposure and invdepth requires a gradient.  The
    inputs are converted to `dtype` on their own device; their gradients arrive in their own dtype."""
    F = torch.nn.functional
    x, y = image.to(dtype), gt.to(dtype)
    C, H, W = x.shape
    if exposure is not None:
        E = exposure.to(dtype)
        x = torch.stack([E[0, c] * x[0] + E[1, c] * x[1] + E[2, c] * x[2] + E[c, 3] for c in range(3)])
    if mask is not None:
        m = mask.to(dtype).reshape(1, H, W)
        x, y = m * x, m * y
    l1 = (x - y).abs().mean()
    g = taps(dtype, x.device)
    w = (g[:, None] @ g[None, :]).expand(C, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t[None], w, padding=5, groups=C)[0]
    mu1, mu2 = conv(x), conv(y)
    s11, s22, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    ssim = (((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s11 + s22 + 9e-4))).mean()
    if invdepth is not None:
        t = invdepth.to(dtype).reshape(H, W) - invdepth_prior.to(dtype).reshape(H, W)
        if invdepth_mask is not None:
            t = t * invdepth_mask.to(dtype).reshape(H, W)
        ld = t.abs().mean()
    else:
        ld = torch.zeros((), dtype=dtype, device=x.device)
    loss = (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - ssim) + invdepth_weight * ld
    return loss, l1, ssim, ld


def loss_and_grads(image, gt, lambda_dssim=0.2, mask=None, exposure=None, invdepth=None, invdepth_prior=None, invdepth_mask=None,
                   invdepth_weight=0.0, dtype=torch.float64):
    """-> (vals (4,) in `dtype`, {"image": ..., "exposure": ..., "invdepth": ...} in `dtype`), the gradients of the inputs given"""
    leaf = lambda t: None if t is None else t.detach().to(dtype).requires_grad_(True)
    x, E, d = leaf(image), leaf(exposure), leaf(invdepth)
    terms = loss_terms(x, gt, lambda_dssim, mask, E, d, invdepth_prior, invdepth_mask, invdepth_weight, dtype)
    terms[0].backward()
    grads = {name: t.grad for name, t in (("image", x), ("exposure", E), ("invdepth", d)) if t is not None}
    return torch.stack([t.detach() for t in terms]), grads
