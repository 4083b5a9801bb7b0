"""A float64 dense autograd restatement of the rasterizer forward that takes the camera as TENSORS: V (viewmatrix), PM (projmatrix)
and campos, each either shared -- (4,4), (4,4), (3,) -- or as one copy per Gaussian -- (P,4,4), (P,4,4), (P,3).  With per-Gaussian
copies autograd yields every Gaussian's own term t_g of a camera gradient as well as the total sum_g t_g, which is what the bar of
tests/test_camera_grads_gpu.py is scaled with.  TEST INFRASTRUCTURE, the camera counterpart of tests/torch_splat.py: the same
function with the same deliberate deviations (straight-through 0.99 clamp; inside the frustum clamp of the EWA Jacobian the clamped
t.x / t.y are constants; masks, tile membership, depth order, culling and radii carry no gradient), plus the opacity compensation of
the screen-space filter (include/gsr_aa.h) and the depth / alpha maps (include/gsr_aux.h).  Discrete decisions are taken from the
oracle state `o` of the same inputs.  `dtype` selects the arithmetic: the float32 run of this very function measures d32."""
import numpy as np
import torch

from torch_splat import sh_color


def _per_gaussian(t, P, tail):
    return t if t.dim() == len(tail) + 1 else t.expand(P, *tail)


def render(o, means3D, scales, rotations, opacities, shs, V, PM, campos, scale_modifier=1.0, colors_precomp=None,
           cov3D_precomp=None, antialiasing=False, depth_mode=None, dtype=torch.float64):
    """-> image (3,H,W) [, depth (H,W), alpha (H,W) when depth_mode is "depth" / "invdepth"].  Gaussian inputs that are not used
    (shs with colors_precomp, scales / rotations with cov3D_precomp) may be None."""
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
    dx = pix[ot, 0][None, :] - pxs
    dy = pix[ot, 1][None, :] - pys
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


def camera_terms(o, inputs, dL, **kw):
    """Per-Gaussian camera terms of the loss sum(outputs * dL) in float64, and the float32 run's totals.
    inputs: dict of the Gaussian tensors of render() (float32 CPU) plus V (4,4), PM (4,4), campos (3,); dL: the upstream gradient(s),
    one tensor per output of render().  -> (total, abs_total, d32): dicts over "V", "PM", "campos" of sum_g t_g, sum_g |t_g| and
    max |float32 total - float64 total|."""
    P = inputs["means3D"].shape[0]
    dL = dL if isinstance(dL, (tuple, list)) else (dL,)
    out = {}
    for dt in (torch.float64, torch.float32):
        cam = {"V": inputs["V"].to(dt).expand(P, 4, 4).clone().requires_grad_(True),
               "PM": inputs["PM"].to(dt).expand(P, 4, 4).clone().requires_grad_(True),
               "campos": inputs["campos"].to(dt).expand(P, 3).clone().requires_grad_(True)}
        g = {k: v for k, v in inputs.items() if k not in cam}
        res = render(o, g["means3D"], g.get("scales"), g.get("rotations"), g["opacities"], g.get("shs"), cam["V"], cam["PM"],
                     cam["campos"], dtype=dt, **kw)
        res = res if isinstance(res, tuple) else (res,)
        loss = sum((r * d.to(dt).reshape(r.shape)).sum() for r, d in zip(res, dL))
        grads = torch.autograd.grad(loss, list(cam.values()), allow_unused=True)
        out[dt] = {k: (torch.zeros_like(cam[k]) if gr is None else gr).to(torch.float64) for k, gr in zip(cam, grads)}
    total = {k: v.sum(0) for k, v in out[torch.float64].items()}
    abs_total = {k: v.abs().sum(0) for k, v in out[torch.float64].items()}
    d32 = {k: float((out[torch.float32][k].sum(0) - total[k]).abs().max()) for k in total}
    return total, abs_total, d32


def camera_test_scene(P=200, W=40, H=24, seed=5):
    """The scene of the camera-gradient tests: P random Gaussians of SH degree 3 in front of a 40 x 24 camera (one full tile column
    plus a ragged edge), some of them moved behind the near plane or far outside the frustum (culled), some placed close to the camera
    and off its axis (frustum clamp of the EWA Jacobian active), one enlarged so that it covers every tile, one shrunk below a pixel.
    -> (scene, cam)"""
    import gsr_scene
    scene = gsr_scene.make_scene(P, -2.0, sh_degree=3, seed=seed)
    cam = gsr_scene.make_camera(W, H)
    means, scales = scene.means3D.clone(), scene.scales.clone()
    if P >= 40:
        means[0:6, 2] = -6.0                                   # behind the camera at (0, 0, -4)
        means[6:10, 0] = 40.0                                  # far outside the frustum
        g = torch.Generator().manual_seed(seed + 1)
        k = torch.arange(10, 22)                               # close and off-axis: |t.x / t.z| > 1.3 tan(fovx / 2), still touching the image
        means[k, 2] = -3.4
        means[k, 0] = torch.where(torch.rand(12, generator=g) < 0.5, -1.0, 1.0) * (0.45 + 0.1 * torch.rand(12, generator=g))
        means[k, 1] = 0.3 * (torch.rand(12, generator=g) - 0.5)
        scales[k] = 0.25
        scales[22] = 1.5                                       # covers the whole image
        means[22] = torch.tensor([0.1, 0.05, 0.5])
        scales[23] = 1e-3                                      # sub-pixel
        means[23] = torch.tensor([-0.2, 0.1, 0.0])
    return scene._replace(means3D=means, scales=scales), cam
