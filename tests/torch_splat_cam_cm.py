"""A float64 dense autograd restatement of the camera-model forward that takes the camera as TENSORS: V (viewmatrix), campos and the
four intrinsics K = (fx, fy, cx, cy), each either shared -- (4,4), (3,), (4,) -- or as one copy per Gaussian -- (P,4,4), (P,3), (P,4).
With per-Gaussian copies autograd yields every Gaussian's own term t_g of a camera gradient as well as the total sum_g t_g, which is
what the bar of tests/test_cam_cm_gpu.py is scaled with.  TEST INFRASTRUCTURE, the camera-model counterpart of
tests/torch_splat_cam.py: the function of tests/torch_splat_camera_model.py (whose project(), covariance3d(), fisheye_terms(), band()
and scenes it reuses) with the same deliberate deviations -- straight-through 0.99 clamp; inside the pinhole's guard band the clamped
t.x / t.y are constants and the band's limits carry no gradient with respect to the intrinsics; masks, tile membership, depth
order, culling and radii carry no gradient.  The discrete decisions are the `state` of a torch_splat_camera_model.render() run on the
same inputs.  `dtype` selects the arithmetic: the float32 run of this very function measures d32.

`keep`, a dict, receives the intermediates the closed forms of DESIGN 6o are written in (each with retain_grad): t (P,3) the
view-space mean, pix (P,2), J (P,2,3), JW = J W (P,2,3) and dirv = mean - campos (P,3)."""
import math

import numpy as np
import torch

import torch_splat_camera_model as tcm
from torch_splat import sh_color


def _per_gaussian(t, P, tail):
    return t if t.dim() == len(tail) + 1 else t.expand(P, *tail)


def render(model, W, H, bg, D, state, means3D, opacities, V, campos, K, scales=None, rotations=None, shs=None, colors_precomp=None,
           cov3D_precomp=None, scale_modifier=1.0, antialiasing=False, depth_mode=None, dtype=torch.float64, means2D=None, keep=None):
    """-> dict: image (3,H,W); depth, alpha (H,W) with depth_mode "depth" / "invdepth".  model: "pinhole" / "fisheye"; K: the tensor
    (fx, fy, cx, cy); state: of torch_splat_camera_model.render() on the same inputs; means2D: as there."""
    dt = dtype
    c = lambda t: None if t is None else t.to(dt)
    means3D, opacities, V, campos, K, scales, rotations, shs, colors_precomp, cov3D_precomp, bg = map(
        c, (means3D, opacities, V, campos, K, scales, rotations, shs, colors_precomp, cov3D_precomp, bg))
    P = means3D.shape[0]
    Vp, cp, Kp = _per_gaussian(V, P, (4, 4)), _per_gaussian(campos, P, (3,)), _per_gaussian(K, P, (4,))
    hom = torch.cat([means3D, torch.ones(P, 1, dtype=dt)], 1)
    t = torch.einsum("pi,pij->pj", hom, Vp)[:, :3]          # flat index 4 * c + r: t_j = sum_i hom_i V[i][j]
    tz = t[:, 2]
    front = tz.detach() > 0.2
    ts = torch.where(front[:, None], t, torch.tensor([0.0, 0.0, 1.0], dtype=dt).expand(P, 3))   # culled: a harmless stand-in
    pix, J, _ = tcm.project((model, Kp[:, 0], Kp[:, 1], Kp[:, 2], Kp[:, 3]), ts, W, H)
    if means2D is not None:
        pix = pix + means2D.to(dt)[:, :2] * torch.tensor([0.5 * W, 0.5 * H], dtype=dt)
    Sigma = tcm.covariance3d(scales, rotations, scale_modifier, cov3D_precomp)
    JW = J @ Vp[:, :3, :3].transpose(1, 2)                  # world -> view rotation, per Gaussian
    dirv = means3D - cp
    if keep is not None:
        for name, v in (("t", t), ("pix", pix), ("J", J), ("JW", JW), ("dirv", dirv)):
            if v.requires_grad:
                v.retain_grad()
            keep[name] = v
    cov = JW @ Sigma @ JW.transpose(1, 2)
    a0, b, c0 = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    a, cc_ = a0 + 0.3, c0 + 0.3
    det = a * cc_ - b * b
    vis, order = state["vis"], state["order"]
    minx, miny, maxx, maxy = (v.numpy().astype(np.int64)[order] for v in state["rect"])
    det = torch.where(vis, det, torch.ones_like(det))
    ca, cb, cc = cc_ / det, -b / det, a / det
    op = opacities.reshape(-1)
    if antialiasing:
        ratio = torch.where(vis, (a0 * c0 - b * b) / det, torch.ones_like(det))
        op = op * torch.sqrt(torch.clamp_min(ratio, 2.5e-5))
    if colors_precomp is not None:
        rgb = colors_precomp
    else:
        rgb = sh_color(D, shs, dirv / dirv.norm(dim=1, keepdim=True))
    ot = torch.from_numpy(order)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    pxs, pys = xs.reshape(-1, 1), ys.reshape(-1, 1)
    txs = (xs.reshape(-1).numpy() // 16).astype(np.int64)[:, None]
    tys = (ys.reshape(-1).numpy() // 16).astype(np.int64)[:, None]
    member = torch.from_numpy((txs >= minx) & (txs < maxx) & (tys >= miny) & (tys < maxy))
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
    out = dict(image=(w @ rgb[ot] + T_final[:, None] * bg[None]).t().reshape(3, H, W))
    if depth_mode is not None:
        v = tz[ot] if depth_mode == "depth" else 1.0 / tz[ot]
        out["depth"], out["alpha"] = (w @ v).reshape(H, W), (1.0 - T_final).reshape(H, W)
    return out


def intrinsics(cm):
    return torch.tensor([float(v) for v in cm[1:]], dtype=torch.float64)


def probe_state(cm, W, H, bg, D, inputs, **kw):
    """The discrete state (and the fragile pixels / radii) of the float64 run of torch_splat_camera_model.render()."""
    with torch.no_grad():
        return tcm.render(cm, W, H, bg, D, V=inputs["V"], campos=inputs["campos"],
                          **{k: v for k, v in inputs.items() if k not in ("V", "campos")}, **kw)["state"]


def _loss(out, dL, dt):
    return sum((out[k] * g.to(dt).reshape(out[k].shape)).sum() for k, g in dL.items())


def camera_terms(cm, W, H, bg, D, inputs, dL, state, want_gaussians=False, **kw):
    """Per-Gaussian camera terms of the loss sum(outputs * dL) in float64, and the float32 run's totals.
    inputs: dict of the Gaussian tensors of render() (float32 CPU) plus V (4,4) and campos (3,); dL: dict over "image" [, "depth",
    "alpha"].  -> (total, abs_total, d32): dicts over "V", "campos", "K" of sum_g t_g, sum_g |t_g| and max |float32 total - float64
    total|; with want_gaussians also the float64 gradients of the Gaussian tensors (fourth element) and the per-Gaussian terms
    themselves (fifth)."""
    P = inputs["means3D"].shape[0]
    out, gg = {}, None
    for dt in (torch.float64, torch.float32):
        cam = {"V": inputs["V"].to(dt).expand(P, 4, 4).clone().requires_grad_(True),
               "campos": inputs["campos"].to(dt).expand(P, 3).clone().requires_grad_(True),
               "K": intrinsics(cm).to(dt).expand(P, 4).clone().requires_grad_(True)}
        g = {k: v.to(dt).clone().requires_grad_(True) for k, v in inputs.items() if k not in cam}
        res = render(cm[0], W, H, bg, D, state, V=cam["V"], campos=cam["campos"], K=cam["K"], dtype=dt, **g, **kw)
        grads = torch.autograd.grad(_loss(res, dL, dt), list(cam.values()) + list(g.values()), allow_unused=True)
        z = lambda gr, like: (torch.zeros_like(like) if gr is None else gr).to(torch.float64)
        out[dt] = {k: z(gr, cam[k]) for k, gr in zip(cam, grads)}
        if dt == torch.float64:
            gg = {k: z(gr, g[k]) for k, gr in zip(g, grads[3:])}
    total = {k: v.sum(0) for k, v in out[torch.float64].items()}
    abs_total = {k: v.abs().sum(0) for k, v in out[torch.float64].items()}
    d32 = {k: float((out[torch.float32][k].sum(0) - total[k]).abs().max()) for k in total}
    if want_gaussians:
        return total, abs_total, d32, gg, out[torch.float64]
    return total, abs_total, d32


def closed_forms(cm, W, H, keep, means3D):
    """The per-Gaussian terms of DESIGN 6o written out, from the gradients autograd left on the intermediates of `keep` (a float64
    run with per-Gaussian or shared camera tensors): -> dict over "V" (P,4,4), "campos" (P,3), "K" (P,4).
      dL/dvm[4k+i] = dt_i mean_k + dL/dW[i][k],  dL/dvm[12+i] = dt_i,  dL/dW[i][k] = J[0][i] dL/dT0k + J[1][i] dL/dT1k
      dL/dcampos = -dm
      dL/dcx = du, dL/dcy = dv; pinhole dL/dfx = dJ00 / z - dJ02 x_c / z^2 + du x / z;
      fisheye dL/dfx = dJ00 (s + x^2 A) + dJ01 x y A - dJ02 x / d^2 + du s x   (fy with row 1)."""
    model, fx, fy, cx, cy = cm
    g = lambda k: torch.zeros_like(keep[k]) if keep[k].grad is None else keep[k].grad
    t, J = keep["t"].detach(), keep["J"].detach()
    dt_, dpix, dJ, dT, ddir = g("t"), g("pix"), g("J"), g("JW"), g("dirv")
    m = means3D.to(torch.float64)
    P = m.shape[0]
    dW = torch.einsum("pri,prk->pik", J, dT)                 # [i][k]
    dV = torch.zeros(P, 4, 4, dtype=torch.float64)
    dV[:, :3, :3] = (dt_[:, :, None] * m[:, None, :] + dW).transpose(1, 2)   # tensor index [k][i] = flat 4 k + i
    dV[:, 3, :3] = dt_
    x, y, z = t[:, 0], t[:, 1], t[:, 2]
    du, dv = dpix[:, 0], dpix[:, 1]
    if model == "fisheye":
        s, A, _ = tcm.fisheye_terms(x, y, z)
        id2 = 1.0 / (x * x + y * y + z * z)
        dfx = dJ[:, 0, 0] * (s + x * x * A) + dJ[:, 0, 1] * (x * y * A) - dJ[:, 0, 2] * x * id2 + du * s * x
        dfy = dJ[:, 1, 0] * (x * y * A) + dJ[:, 1, 1] * (s + y * y * A) - dJ[:, 1, 2] * y * id2 + dv * s * y
    else:
        (lox, hix), (loy, hiy) = tcm.band(fx, cx, W), tcm.band(fy, cy, H)
        xc, yc = (x / z).clamp(lox, hix) * z, (y / z).clamp(loy, hiy) * z   # the clamped coordinates, constants
        dfx = dJ[:, 0, 0] / z - dJ[:, 0, 2] * xc / (z * z) + du * x / z
        dfy = dJ[:, 1, 1] / z - dJ[:, 1, 2] * yc / (z * z) + dv * y / z
    return {"V": dV, "campos": -ddir, "K": torch.stack([dfx, dfy, du, dv], 1)}


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def fisheye_points_scene(P=300, W=40, H=24, seed=9):
    """fisheye_scene() with Gaussians at the points where the fisheye's terms are delicate (view space; the camera sits at (0, 0, -4)
    and looks along +z): 24 exactly on the optical axis, 25 at r / z = 1e-4, 26 at theta = 80 degrees, 27 and 28 on either side of
    the series switch q = r^2 / z^2 = 0.1.  -> (scene, cam, cm, dict of the indices)"""
    scene, cam, cm = tcm.fisheye_scene(P, W, H, seed)
    means, scales = scene.means3D.clone(), scene.scales.clone()
    z = 3.6
    means[25] = torch.tensor([0.6e-4 * z, -0.8e-4 * z, z - 4.0])
    means[26] = torch.tensor([-0.5 * math.tan(math.radians(80.0)), 0.0, -3.5])   # view z = 0.5
    r = 3.0 * math.sqrt(tcm.SERIES_Q)
    means[27] = torch.tensor([0.6 * r * (1 - 1e-3), 0.8 * r * (1 - 1e-3), -1.0])  # view z = 3
    means[28] = torch.tensor([-0.8 * r * (1 + 1e-3), 0.6 * r * (1 + 1e-3), -1.0])
    scales[25] = 0.12
    scales[26] = 0.05
    scales[27:29] = 0.1
    return scene._replace(means3D=means, scales=scales), cam, cm, dict(axis=24, near_axis=25, wide=26, below=27, above=28)


def guard_sides_scene(P=300, W=40, H=24, seed=7):
    """guard_scene() -- twelve Gaussians inside the asymmetric guard band, beyond the old symmetric limit -- with three of them moved
    past the band's limit on the long side and three past it on the short side, where the clamp is active; all still touch the image.
    -> (scene, cam, cm, dict: inside, beyond_hi, beyond_lo index tensors)"""
    scene, cam, cm, k = tcm.guard_scene(P, W, H, seed)
    lox, hix = tcm.band(cm[1], cm[3], W)
    means, scales = scene.means3D.clone(), scene.scales.clone()
    zv = 3.4
    hi, lo = k[:3], k[3:6]
    means[hi, 0] = torch.tensor([1.01, 1.03, 1.05]) * hix * zv
    means[lo, 0] = torch.tensor([1.01, 1.03, 1.05]) * lox * zv
    scales[hi] = 0.4
    scales[lo] = 0.4
    return scene._replace(means3D=means, scales=scales), cam, cm, dict(inside=k[6:], beyond_hi=hi, beyond_lo=lo)
