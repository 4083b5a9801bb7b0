"""Absolute screen-space gradients in float64: the reference of tests/test_absgrad_gpu.py.  TEST INFRASTRUCTURE.

render() restates tests/torch_splat_cam.render -- the same dense autograd function with the same deliberate deviations, taken line by
line -- and adds a zero offset of shape (pixels, Gaussians, 2) to the projected means inside dx, dy, so that autograd returns every
pixel's own term dL_p/dmean2D_g instead of their sum.  abs_terms() turns the terms into the quantity of include/gsr_absgrad.h,
0.5 (W, H) sum_p |term| (the projected mean in NDC: pix = ((ndc + 1) S - 1) / 2), beside the signed sum, and measures the float32
rounding of the same function (d32), the project's bar for sums formed in float32."""
import numpy as np
import torch

from torch_splat import sh_color
from torch_splat_cam import _per_gaussian


def render(o, means3D, scales, rotations, opacities, shs, V, PM, campos, scale_modifier=1.0, colors_precomp=None,
           cov3D_precomp=None, antialiasing=False, depth_mode=None, dtype=torch.float64, pixel_offset=None, mean_offset=None):
    """torch_splat_cam.render() with two more inputs: pixel_offset (pixels, P, 2), added to Gaussian g's projected mean as pixel p sees
    it inside dx, dy, and mean_offset (P, 2), added to the projected mean as every pixel sees it (pixel units both).
    -> image (3,H,W) [, depth (H,W), alpha (H,W) when depth_mode is "depth" / "invdepth"]."""
    W, H, D = o["W"], o["H"], o["D"]
    dt = dtype
    c = lambda t: None if t is None else t.to(dt)
    means3D, scales, rotations, opacities, shs, V, PM, campos, colors_precomp, cov3D_precomp = map(
        c, (means3D, scales, rotations, opacities, shs, V, PM, campos, colors_precomp, cov3D_precomp))
    bg = torch.from_numpy(o["bg"]).to(dt)
    tanx, tany = o["tanfovx"], o["tanfovy"]
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    P = means3D.shape[0]
    Vp, PMp, cp = _per_gaussian(V, P, (4, 4)), _per_gaussian(PM, P, (4, 4)), _per_gaussian(campos, P, (3,))
    hom = torch.cat([means3D, torch.ones(P, 1, dtype=dt)], 1)
    t = torch.einsum("pi,pij->pj", hom, Vp)[:, :3]          # flat index 4 * c + r: t_j = sum_i hom_i V[i][j]
    ph = torch.einsum("pi,pij->pj", hom, PMp)
    pw = 1.0 / (ph[:, 3] + 1e-7)
    ndc = ph[:, :2] * pw[:, None]
    pix = torch.stack([((ndc[:, 0] + 1.0) * W - 1.0) * 0.5, ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5], 1)
    vis = torch.from_numpy(o["radii"] > 0)
    tz = t[:, 2]
    limx, limy = 1.3 * tanx, 1.3 * tany
    in_x = ((t[:, 0] / tz).detach().abs() <= limx)
    in_y = ((t[:, 1] / tz).detach().abs() <= limy)
    tx = torch.where(in_x, t[:, 0], (torch.sign(t[:, 0]) * limx * tz).detach())
    ty = torch.where(in_y, t[:, 1], (torch.sign(t[:, 1]) * limy * tz).detach())
    render.clamp_active = int(((~in_x | ~in_y) & vis).sum())
    if cov3D_precomp is not None:
        s6 = cov3D_precomp
        Sigma = torch.stack([s6[:, 0], s6[:, 1], s6[:, 2], s6[:, 1], s6[:, 3], s6[:, 4], s6[:, 2], s6[:, 4], s6[:, 5]], 1).reshape(P, 3, 3)
    else:
        r, x, y, z = rotations[:, 0], rotations[:, 1], rotations[:, 2], rotations[:, 3]
        Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                          2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                          2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(P, 3, 3)
        S = torch.diag_embed(scales + (scale_modifier - 1.0) * scales.detach())
        Mm = Rm @ S
        Sigma = Mm @ Mm.transpose(1, 2)
    Wm = Vp[:, :3, :3].transpose(1, 2)                      # world -> view rotation, per Gaussian
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -fx * tx / (tz * tz), zero, fy / tz, -fy * ty / (tz * tz)], 1).reshape(P, 2, 3)
    JW = J @ Wm
    cov = JW @ Sigma @ JW.transpose(1, 2)
    a0, b, c0 = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    # visible Gaussians whose undilated footprint is below a pixel: both variances under 0.25 px^2 (sigma < 0.5 px)
    render.subpixel = int((vis & (a0.detach() < 0.25) & (c0.detach() < 0.25)).sum())
    a, cc_ = a0 + 0.3, c0 + 0.3
    det = a * cc_ - b * b
    det = torch.where(vis, det, torch.ones_like(det))
    ca, cb, cc = cc_ / det, -b / det, a / det
    op = opacities.reshape(-1)
    if antialiasing:   # include/gsr_aa.h: rho = sqrt(max(2.5e-5, N / Dh)); the clamp's flat side carries no gradient, as max() has none
        ratio = (a0 * c0 - b * b) / det
        ratio = torch.where(vis, ratio, torch.ones_like(ratio))
        op = op * torch.sqrt(torch.clamp_min(ratio, 2.5e-5))
    if colors_precomp is not None:
        rgb = colors_precomp
    else:
        d = means3D - cp
        d = d / d.norm(dim=1, keepdim=True)
        rgb = sh_color(D, shs, d)

    order = np.lexsort((np.arange(P), o["depths"]))
    order = order[o["radii"][order] > 0]
    ot = torch.from_numpy(order)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    pxs, pys = xs.reshape(-1, 1), ys.reshape(-1, 1)
    m2, rad = o["means2D"][order], o["radii"][order]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    f2i = lambda v: np.trunc(v).astype(np.int64)
    minx = np.clip(f2i((m2[:, 0] - rad) / np.float32(16)), 0, gx)
    miny = np.clip(f2i((m2[:, 1] - rad) / np.float32(16)), 0, gy)
    maxx = np.clip(f2i((m2[:, 0] + rad + 15) / np.float32(16)), 0, gx)
    maxy = np.clip(f2i((m2[:, 1] + rad + 15) / np.float32(16)), 0, gy)
    txs = (xs.reshape(-1).numpy() // 16).astype(np.int64)[:, None]
    tys = (ys.reshape(-1).numpy() // 16).astype(np.int64)[:, None]
    member = torch.from_numpy((txs >= minx) & (txs < maxx) & (tys >= miny) & (tys < maxy))
    render.max_tiles = int(((maxx - minx) * (maxy - miny)).max()) if len(order) else 0
    if mean_offset is not None:
        pix = pix + mean_offset.to(dt)
    dx = pix[ot, 0][None, :] - pxs
    dy = pix[ot, 1][None, :] - pys
    if pixel_offset is not None:
        dx = dx + pixel_offset.to(dt)[:, ot, 0]
        dy = dy + pixel_offset.to(dt)[:, ot, 1]
    power = -0.5 * (ca[ot][None] * dx * dx + cc[ot][None] * dy * dy) - cb[ot][None] * dx * dy
    G = torch.exp(power)
    oG = op[ot][None] * G
    alpha = oG + (torch.clamp(oG, max=0.99) - oG).detach()
    live = member & (power.detach() <= 0) & (alpha.detach() >= 1.0 / 255.0)
    one_m = torch.where(live, 1.0 - alpha, torch.ones_like(alpha))
    Tincl = torch.cumprod(one_m, dim=1)
    Texcl = torch.cat([torch.ones(Tincl.shape[0], 1, dtype=dt), Tincl[:, :-1]], 1)
    stop = live & (Tincl.detach() < 1e-4)
    stopped = torch.cumsum(stop.to(torch.int64), dim=1) > 0
    valid = live & ~stopped
    w = torch.where(valid, alpha * Texcl, torch.zeros_like(alpha))
    T_final = torch.prod(torch.where(valid, 1.0 - alpha, torch.ones_like(alpha)), dim=1)
    img = (w @ rgb[ot] + T_final[:, None] * bg[None]).t().reshape(3, H, W)
    if depth_mode is None:
        return img
    v = tz[ot] if depth_mode == "depth" else 1.0 / tz[ot]
    return img, (w @ v).reshape(H, W), (1.0 - T_final).reshape(H, W)


def abs_terms(o, inputs, dL, **kw):
    """inputs: dict of the Gaussian tensors of render() (float32 CPU) plus V (4,4), PM (4,4), campos (3,); dL: the upstream gradient(s),
    one tensor per output of render().  -> (ref [P, 2] = 0.5 (W, H) sum_p |t_p|, signed [P, 2] = 0.5 (W, H) sum_p t_p, both float64,
    d32 = per component max_g |float32 run's ref - ref|)."""
    P = inputs["means3D"].shape[0]
    W, H = o["W"], o["H"]
    dL = dL if isinstance(dL, (tuple, list)) else (dL,)
    res = {}
    for dt in (torch.float64, torch.float32):
        off = torch.zeros(W * H, P, 2, dtype=dt, requires_grad=True)
        g = inputs
        out = render(o, g["means3D"], g.get("scales"), g.get("rotations"), g["opacities"], g.get("shs"), g["V"], g["PM"], g["campos"],
                     dtype=dt, pixel_offset=off, **kw)
        out = out if isinstance(out, tuple) else (out,)
        loss = sum((r * d.to(dt).reshape(r.shape)).sum() for r, d in zip(out, dL))
        t, = torch.autograd.grad(loss, [off])
        scale = torch.tensor([0.5 * W, 0.5 * H], dtype=dt)
        res[dt] = (t.abs().sum(0) * scale, t.sum(0) * scale)
    ref, signed = res[torch.float64]
    d32 = (res[torch.float32][0].to(torch.float64) - ref).abs().max(0).values
    return ref, signed, d32
