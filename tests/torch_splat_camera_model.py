"""A dense autograd restatement of the rasterizer forward for the camera models of include/gsr_camera_model.h: tests/torch_splat.py
with the projection and the EWA Jacobian of a CameraModel -- "pinhole" with intrinsics (asymmetric guard band) or "fisheye"
(equidistant).  TEST INFRASTRUCTURE.  Gradients come from torch.autograd, so they are derived independently of the hand-written
second derivatives in csrc/gsr_camera_model.h.  The deliberate deviations from the true gradient are those of tests/torch_splat.py
(straight-through 0.99 clamp; inside the pinhole's guard band the clamped t.x / t.y are constants; dL/dscale without the
scale_modifier factor; masks, tile membership, depth order, culling and radii carry no gradient).

It needs no oracle state: radii, tile rectangles, depth order and the accept / reject masks are computed here, in float64 (`state`
of the float64 run; the float32 run, which measures d32, takes the discrete part of that state).  It also returns
  fragile         per pixel: an accept / reject decision (alpha >= 1/255, power <= 0, T < 1e-4) taken within `margin` of its threshold,
                  with the oracle's definition (oracle/gsr_oracle.c) and util.oracle_forward's default margin 2e-5
  fragile_radius  per Gaussian: 3 sqrt(lambda) within 1e-4 of an integer, or a rectangle edge within 1e-4 px of a tile boundary
"""
import numpy as np
import torch

from torch_splat import sh_color

SERIES_Q = 0.1       # GSR_CM_SERIES_Q: below this r^2 / z^2 the fisheye terms come from their Taylor series
SERIES_TERMS = 10    # GSR_CM_SERIES_TERMS


def series(q, kind):
    """Horner evaluation, highest power first, of the ten-term series in q = r^2 / z^2 (csrc/gsr_camera_model.h; eleven terms for
    "s", whose derivative is then the series of "A" term by term):
    "s": z s = sum_k (-1)^k q^k / (2k+1);  "A": z^3 A = sum_{k>=1} (-1)^k 2k / (2k+1) q^(k-1);
    "Ar2": z^5 dA/d(r^2) = sum_{k>=2} (-1)^k 2k (k-1) / (2k+1) q^(k-2)."""
    p = torch.zeros_like(q)
    for k in reversed(range(SERIES_TERMS + (kind == "s"))):
        sign = -1.0 if k & 1 else 1.0
        if kind == "s":
            c = sign / (2 * k + 1)
        elif kind == "A":
            c = -sign * (2 * (k + 1)) / (2 * (k + 1) + 1)
        else:
            c = sign * (2 * (k + 2) * (k + 1)) / (2 * (k + 2) + 1)
        p = p * q + c
    return p


def fisheye_terms(x, y, z, force=None):
    """-> (s, A, Ar2) of the equidistant fisheye at the view-space point (x, y, z), in the dtype of the inputs:
    s = theta / r, A = (z / d2 - s) / r^2 (ds/dx = x A), Ar2 = dA/d(r^2).  force: None = the kernel's switch at SERIES_Q,
    "series" / "closed" = that form everywhere (the closed form is 0/0 on the axis)."""
    r2, z2 = x * x + y * y, z * z
    d2 = r2 + z2
    q = r2 / z2
    near = (q < SERIES_Q) if force is None else torch.full_like(q, force == "series", dtype=torch.bool)
    s_s, A_s, R_s = series(q, "s") / z, series(q, "A") / (z * z2), series(q, "Ar2") / (z * z2 * z2)
    r2c = torch.where(near, torch.ones_like(r2), r2)   # (keeps the unselected closed form finite, for autograd)
    r = torch.sqrt(r2c)
    s_c = torch.atan2(r, z) / r
    A_c = (z / d2 - s_c) / r2c
    R_c = (-(z / (d2 * d2)) - 1.5 * A_c) / r2c
    return torch.where(near, s_s, s_c), torch.where(near, A_s, A_c), torch.where(near, R_s, R_c)


def band(f, c, S):
    """the pinhole's guard band along one axis: t.x / t.z is clamped to [lo, hi] inside the Jacobian"""
    m = 0.3 * S / (2.0 * f)
    return -(c / f + m), (S - c) / f + m


def project(cm, t, W, H, force=None):
    """-> (pix (P,2), J (P,2,3), in_band (P,) bool): the pixel-index mean u = projected x + cx - 0.5 and the analytic Jacobian the
    covariance is projected with (the pinhole's with the guard band's clamp as a constant), differentiable in t."""
    model, fx, fy, cx, cy = cm
    x, y, z = t[:, 0], t[:, 1], t[:, 2]
    zero = torch.zeros_like(z)
    if model == "fisheye":
        s, A, _ = fisheye_terms(x, y, z, force)
        pix = torch.stack([fx * s * x + (cx - 0.5), fy * s * y + (cy - 0.5)], 1)
        d2 = x * x + y * y + z * z
        J = torch.stack([fx * (s + x * x * A), fx * x * y * A, -fx * x / d2,
                         fy * x * y * A, fy * (s + y * y * A), -fy * y / d2], 1).reshape(-1, 2, 3)
        return pix, J, torch.ones_like(z, dtype=torch.bool)
    if model != "pinhole":
        raise ValueError(model)
    pix = torch.stack([fx * x / z + (cx - 0.5), fy * y / z + (cy - 0.5)], 1)
    (lox, hix), (loy, hiy) = band(fx, cx, W), band(fy, cy, H)
    txtz, tytz = (x / z).detach(), (y / z).detach()
    in_x, in_y = (txtz >= lox) & (txtz <= hix), (tytz >= loy) & (tytz <= hiy)
    tx = torch.where(in_x, x, (txtz.clamp(lox, hix) * z).detach())
    ty = torch.where(in_y, y, (tytz.clamp(loy, hiy) * z).detach())
    J = torch.stack([fx / z, zero, -fx * tx / (z * z), zero, fy / z, -fy * ty / (z * z)], 1).reshape(-1, 2, 3)
    return pix, J, in_x & in_y


def default_model(W, H, tanfovx, tanfovy):
    return ("pinhole", W / (2.0 * tanfovx), H / (2.0 * tanfovy), W / 2.0, H / 2.0)


def covariance3d(scales, rotations, scale_modifier, cov3D_precomp):
    if cov3D_precomp is not None:
        s6 = cov3D_precomp
        return torch.stack([s6[:, 0], s6[:, 1], s6[:, 2], s6[:, 1], s6[:, 3], s6[:, 4], s6[:, 2], s6[:, 4], s6[:, 5]], 1).reshape(-1, 3, 3)
    r, x, y, z = rotations[:, 0], rotations[:, 1], rotations[:, 2], rotations[:, 3]
    Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                      2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                      2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    S = torch.diag_embed(scales + (scale_modifier - 1.0) * scales.detach())
    Mm = Rm @ S
    return Mm @ Mm.transpose(1, 2)


def render(cm, W, H, bg, D, means3D, opacities, V, campos, scales=None, rotations=None, shs=None, colors_precomp=None,
           cov3D_precomp=None, scale_modifier=1.0, antialiasing=False, depth_mode=None, dtype=torch.float64, state=None, margin=2e-5,
           detach_pix=False, means2D=None):
    """-> dict: image (3,H,W); depth, alpha (H,W) with depth_mode "depth" / "invdepth"; state.  V: viewmatrix (4,4) in the flat
    4 * c + r convention of the settings (t = [mean, 1] @ V); inputs are CPU tensors of any float dtype and are converted to `dtype`.
    state: None = take every discrete decision here (the float64 run); else the state of that run, whose radii, rectangles and
    depth order are used (the float32 run).  detach_pix: the pixel mean carries no gradient -- what is left of dL/dmeans3D is the part
    through the 2D covariance (and the SH direction and the depth value).  means2D: (P, 3) zeros, the carrier of the screen-space
    gradient: its gradient is (0.5 W dL/du, 0.5 H dL/dv, 0), the units of the rasterizer's means2D.grad."""
    dt = dtype
    c = lambda t: None if t is None else t.to(dt)
    means3D, opacities, V, campos, scales, rotations, shs, colors_precomp, cov3D_precomp, bg = map(
        c, (means3D, opacities, V, campos, scales, rotations, shs, colors_precomp, cov3D_precomp, bg))
    P = means3D.shape[0]
    hom = torch.cat([means3D, torch.ones(P, 1, dtype=dt)], 1)
    t = (hom @ V)[:, :3]
    tz = t[:, 2]
    front = tz.detach() > 0.2
    ts = torch.where(front[:, None], t, torch.tensor([0.0, 0.0, 1.0], dtype=dt).expand(P, 3))   # culled: a harmless stand-in
    pix, J, in_band = project(cm, ts, W, H)
    if detach_pix:
        pix = pix.detach()
    if means2D is not None:
        pix = pix + means2D.to(dt)[:, :2] * torch.tensor([0.5 * W, 0.5 * H], dtype=dt)
    Sigma = covariance3d(scales, rotations, scale_modifier, cov3D_precomp)
    JW = J @ V[:3, :3].t()
    cov = JW @ Sigma @ JW.transpose(1, 2)
    a0, b, c0 = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    a, cc_ = a0 + 0.3, c0 + 0.3
    det = a * cc_ - b * b
    gx, gy = (W + 15) // 16, (H + 15) // 16
    if state is None:
        d64 = det.detach().double()
        mid = 0.5 * (a + cc_).detach().double()
        lam = mid + torch.sqrt(torch.clamp_min(mid * mid - d64, 0.1))
        r3 = 3.0 * torch.sqrt(lam)
        rad = torch.ceil(r3)
        px, py = pix[:, 0].detach().double(), pix[:, 1].detach().double()
        edges = torch.stack([px - rad, px + rad + 15.0, py - rad, py + rad + 15.0], 1)
        tr = torch.trunc(edges / 16.0)
        minx, maxx = tr[:, 0].clamp(0, gx), tr[:, 1].clamp(0, gx)
        miny, maxy = tr[:, 2].clamp(0, gy), tr[:, 3].clamp(0, gy)
        vis = front & (d64 != 0) & ((maxx - minx) * (maxy - miny) > 0)
        near_tile = ((edges - 16.0 * torch.round(edges / 16.0)).abs() < 1e-4).any(1)
        # (an edge far outside the image cannot move the clamped rectangle)
        inside = ((edges[:, :2] > -16.0) & (edges[:, :2] < 16.0 * (gx + 1))).any(1) | ((edges[:, 2:] > -16.0) & (edges[:, 2:] < 16.0 * (gy + 1))).any(1)
        fragile_radius = front & (((r3 - torch.round(r3)).abs() < 1e-4) | (near_tile & inside) | ((tz.detach().double() - 0.2).abs() < 1e-6))
        depth32 = tz.detach().to(torch.float32).numpy()
        order = np.lexsort((np.arange(P), depth32))
        order = order[vis.numpy()[order]]
        state = dict(vis=vis, radii=torch.where(vis, rad, torch.zeros_like(rad)).to(torch.int32), rect=(minx, miny, maxx, maxy), order=order,
                     fragile_radius=fragile_radius, in_band=in_band, pix=pix.detach().double(), t=t.detach().double(), depth32=depth32,
                     J=J.detach().double())
        first = True
    else:
        first = False
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
        d = means3D - campos
        d = d / d.norm(dim=1, keepdim=True)
        rgb = sh_color(D, shs, d)
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
    pos = member & (power.detach() <= 0)
    live = pos & (alpha.detach() >= 1.0 / 255.0)
    one_m = torch.where(live, 1.0 - alpha, torch.ones_like(alpha))
    Tincl = torch.cumprod(one_m, dim=1)
    Texcl = torch.cat([torch.ones(Tincl.shape[0], 1, dtype=dt), Tincl[:, :-1]], 1)
    stop = live & (Tincl.detach() < 1e-4)
    stopped = torch.cumsum(stop.to(torch.int64), dim=1) > 0
    valid = live & ~stopped
    w = torch.where(valid, alpha * Texcl, torch.zeros_like(alpha))
    T_final = torch.prod(torch.where(valid, 1.0 - alpha, torch.ones_like(alpha)), dim=1)
    out = dict(image=(w @ rgb[ot] + T_final[:, None] * bg[None]).t().reshape(3, H, W), state=state)
    if depth_mode is not None:
        v = tz[ot] if depth_mode == "depth" else 1.0 / tz[ot]
        out["depth"], out["alpha"] = (w @ v).reshape(H, W), (1.0 - T_final).reshape(H, W)
    if first:
        # decisions the blend of a pixel actually reaches: up to and including the one that stops it
        reached = member & ~(torch.cumsum(stop.to(torch.int64), dim=1) - stop.to(torch.int64) > 0)
        pw, al, tt = power.detach(), alpha.detach(), Tincl.detach()
        frag = reached & (pw.abs() < margin)
        frag |= reached & (pw <= 0) & ((al - 1.0 / 255.0).abs() < margin * (1.0 / 255.0))
        frag |= reached & live & ((tt - 1e-4).abs() < margin * 1e-4)
        state["fragile"] = frag.any(1).reshape(H, W)
        state["weights"] = w.detach()
    return out


def loss_and_grads(cm, W, H, bg, D, inputs, dL, dtype=torch.float64, state=None, **kw):
    """inputs: dict of the Gaussian tensors of render() (float32 CPU tensors) plus V and campos; dL: dict over "image" [, "depth",
    "alpha"] of upstream gradients.  -> (out of render(), dict of gradients w.r.t. every Gaussian tensor, in float64)"""
    diff = {k: v.to(dtype).clone().requires_grad_(True) for k, v in inputs.items() if k not in ("V", "campos")}
    out = render(cm, W, H, bg, D, V=inputs["V"], campos=inputs["campos"], dtype=dtype, state=state, **diff, **kw)
    loss = sum((out[k] * g.to(dtype).reshape(out[k].shape)).sum() for k, g in dL.items())
    grads = torch.autograd.grad(loss, list(diff.values()), allow_unused=True)
    return out, {k: (torch.zeros_like(v) if g is None else g).detach().to(torch.float64) for (k, v), g in zip(diff.items(), grads)}


def reference(cm, W, H, bg, D, inputs, make_dL, **kw):
    """The float64 run, then the float32 run on its discrete state with the same upstream gradients.
    make_dL(state) -> dL dict (zero on fragile pixels).  -> (out64, grads64, d32 dict of max |float32 - float64| per tensor, dL);
    d32["_split"] holds split_sample() of the float32 run."""
    with torch.no_grad():
        probe = render(cm, W, H, bg, D, V=inputs["V"], campos=inputs["campos"],
                       **{k: v for k, v in inputs.items() if k not in ("V", "campos")}, **kw)
    dL = make_dL(probe["state"])
    out64, g64 = loss_and_grads(cm, W, H, bg, D, inputs, dL, torch.float64, probe["state"], **kw)
    g32_of = lambda d: loss_and_grads(cm, W, H, bg, D, inputs, d, torch.float32, probe["state"], **kw)[1]
    g32 = g32_of(dL)
    d32 = {k: float((g32[k] - g64[k]).abs().max()) for k in g64}
    d32["_split"] = split_sample(g32_of, dL, g32)   # (see split_sample: the float32 helper's own reproducibility, for CHAIN)
    return out64, g64, d32, dL


CHAIN = ("scales", "rotations", "scaling", "rotation")   # the gradients at the end of the covariance chain


def split_sample(grads_of, dL, single, seed=99):
    """One sample of a gradient computation's own reproducibility: the upstream gradient split at random into two parts, two backward
    passes added, against the single pass -- equal in exact arithmetic.  grads_of(dL) -> dict of gradients (the float32 helper);
    -> dict of max |two passes - one pass| / max |one pass|.  The bar of the covariance chain's gradients (CHAIN) is widened to
    max(5e-5, 10 x this sample) of the largest element, as tests/test_antialias_gpu.py and tests/test_depth_alpha_gpu.py do."""
    g = torch.Generator().manual_seed(seed)
    parts = {k: v * torch.rand(v.shape, generator=g) for k, v in dL.items()}
    ga, gb = grads_of(parts), grads_of({k: dL[k] - parts[k] for k in dL})
    return {k: float((ga[k] + gb[k] - single[k]).abs().max()) / max(float(single[k].abs().max()), 1e-30) for k in single}


def pinhole_standin(cm, W, H, tanfovx, tanfovy, means3D, V, Sigma_world):
    """The centred-pinhole stand-in of every Gaussian under camera model `cm`, in float64: world-space means and 3D covariances
    (P, 6) whose projection by the core camera (tanfovx, tanfovy, view matrix V) is the splat of `cm` -- pixel mean (u, v), 2D
    covariance J Sigma_view J^T -- at the same view depth.  -> (means (P,3), cov6 (P,6), in_core_band (P,) bool)"""
    dt = torch.float64
    means3D, V, Sigma_world = means3D.to(dt), V.to(dt), Sigma_world.to(dt)
    P = means3D.shape[0]
    fx0, fy0 = W / (2.0 * tanfovx), H / (2.0 * tanfovy)
    t = (torch.cat([means3D, torch.ones(P, 1, dtype=dt)], 1) @ V)[:, :3]
    front = t[:, 2] > 0.2
    ts = torch.where(front[:, None], t, torch.tensor([0.0, 0.0, 1.0], dtype=dt).expand(P, 3))
    pix, J, _ = project(cm, ts, W, H)
    z = ts[:, 2]
    tv = torch.stack([(pix[:, 0] - (W - 1) / 2.0) * z / fx0, (pix[:, 1] - (H - 1) / 2.0) * z / fy0, z], 1)
    Wm = V[:3, :3].t()                       # world -> view rotation
    C = (J @ Wm) @ Sigma_world @ (J @ Wm).transpose(1, 2)
    B = torch.zeros(P, 3, 2, dtype=dt)
    B[:, 0, 0], B[:, 1, 1] = z / fx0, z / fy0
    Sv = B @ C @ B.transpose(1, 2)           # view space
    Sw = Wm.t() @ Sv @ Wm                    # world space
    Vinv = torch.linalg.inv(V)
    mw = (torch.cat([tv, torch.ones(P, 1, dtype=dt)], 1) @ Vinv)[:, :3]
    mw = torch.where(front[:, None], mw, means3D)   # culled Gaussians stay where they are (behind the near plane)
    cov6 = torch.stack([Sw[:, 0, 0], Sw[:, 0, 1], Sw[:, 0, 2], Sw[:, 1, 1], Sw[:, 1, 2], Sw[:, 2, 2]], 1)
    in_core = ((tv[:, 0] / z).abs() <= 1.3 * tanfovx) & ((tv[:, 1] / z).abs() <= 1.3 * tanfovy)
    return mw, cov6, in_core | ~front


# ---- the scenes of tests/test_camera_model_gpu.py; their conditions are asserted on the CPU from this helper alone ---------------------
def base_scene(P=300, W=40, H=24, seed=5, mu=-2.0):
    """P random Gaussians of SH degree 3 in front of the camera at (0, 0, -4), ten of them behind the near plane, two far off the
    image, one enlarged so that it covers every tile, one shrunk below a pixel."""
    import gsr_scene
    scene = gsr_scene.make_scene(P, mu, sh_degree=3, seed=seed)
    cam = gsr_scene.make_camera(W, H)
    means, scales = scene.means3D.clone(), scene.scales.clone()
    if P >= 40:
        means[0:10, 2] = -6.0                                  # behind the camera
        means[10:12, 1] = 40.0                                 # far outside the image
        scales[22] = 1.5                                       # covers the whole image
        means[22] = torch.tensor([0.1, 0.05, 0.5])
        scales[23] = 1e-3                                      # sub-pixel
        means[23] = torch.tensor([-0.2, 0.1, 0.0])
    return scene._replace(means3D=means, scales=scales), cam


def guard_scene(P=300, W=40, H=24, seed=7):
    """base_scene() seen by an off-centre pinhole (cx = 0.3 W, the focal lengths of the centred camera), with twelve Gaussians close to
    the camera between the old symmetric guard limit 1.3 tanfovx and the new one on the long side, (W - cx) / fx + 0.3 W / (2 fx),
    still touching the image.  -> (scene, cam, cm, indices of the twelve)"""
    scene, cam = base_scene(P, W, H, seed)
    fx, fy = W / (2.0 * cam.tanfovx), H / (2.0 * cam.tanfovy)
    cm = ("pinhole", fx, fy, 0.3 * W, 0.5 * H)
    means, scales = scene.means3D.clone(), scene.scales.clone()
    k = torch.arange(30, 42)
    g = torch.Generator().manual_seed(seed + 1)
    zv = 3.4
    means[k, 0] = (0.72 + 0.08 * torch.rand(12, generator=g)) * zv
    means[k, 1] = 0.6 * (torch.rand(12, generator=g) - 0.5)
    means[k, 2] = zv - 4.0
    scales[k] = 0.25
    return scene._replace(means3D=means, scales=scales), cam, cm, k


def crop_scene(P=600, seed=11):
    """A centred 120 x 108 render and its 88 x 60 crop at (32, 48): the crop is the off-centre pinhole cx = 60 - 32, cy = 54 - 48 with
    the same focal lengths.  A Gaussian is visible when its rectangle touches a TILE, and the last tiles overhang the image (8 and 4
    px here), so the guard band's margin of 0.15 W resp. 0.15 H px must exceed overhang + radius: Gaussians of at most 3 px radius and
    these sizes leave no visible Gaussian in either camera's band.  -> (scene, big camera, (W, H), (x0, y0), cm)"""
    import gsr_scene
    scene = gsr_scene.make_scene(P, -4.0, sh_degree=3, seed=seed)
    scene = scene._replace(scales=scene.scales.clamp(max=0.015))
    cam = gsr_scene.make_camera(120, 108)
    fx, fy = 120 / (2.0 * cam.tanfovx), 108 / (2.0 * cam.tanfovy)
    return scene, cam, (88, 60), (32, 48), ("pinhole", fx, fy, 60.0 - 32.0, 54.0 - 48.0)


FISHEYE = ("fisheye", 14.0, 14.0, 20.4, 11.7)
PINHOLE_OFFCENTRE = ("pinhole", 35.0, 33.0, 17.3, 14.1)   # for the 40 x 24 camera of base_scene()
EDGE_SHAPES = ((40, 24), (37, 21), (120, 90))             # one full tile column plus ragged edges; no multiple of 16; many tiles


FISHEYE_PIN = ("fisheye", 30.0, 30.0, 44.3, 29.6)          # for the 88 x 60 camera of the oracle pin


def fisheye_scene(P=300, W=40, H=24, seed=9, cm=None, max_scale=None):
    """base_scene() for the fisheye FISHEYE, with one Gaussian exactly on the optical axis (index 24), one with r / z = 1e-2, far below
    the series threshold (25), and one at theta = 76 degrees (26).  -> (scene, cam, cm)"""
    scene, cam = base_scene(P, W, H, seed)
    means, scales = scene.means3D.clone(), scene.scales.clone()
    if P >= 40:
        means[24] = torch.tensor([0.0, 0.0, 0.3])
        means[25] = torch.tensor([0.03, -0.02, -0.4])
        means[26] = torch.tensor([2.0, 0.1, -3.5])             # view z = 0.5, r = 2.0
        scales[24:26] = 0.12
        scales[26] = 0.05
        if max_scale is not None:
            scales[24:27] = scales[24:27].clamp(max=max_scale)
    return scene._replace(means3D=means, scales=scales), cam, (FISHEYE if cm is None else cm)


def oracle_pin_scene():
    """fisheye_scene() on 88 x 60 with FISHEYE_PIN and small Gaussians, for the pin against the CPU oracle by composition"""
    return fisheye_scene(300, 88, 60, 9, FISHEYE_PIN, 0.08)


def scene_inputs(scene, cam, variant="sh"):
    """The helper's inputs of a scene for a variant of the GPU tests: "sh" | "colors" (colors_precomp) | "cov" (cov3D_precomp)."""
    inp = dict(means3D=scene.means3D, means2D=torch.zeros_like(scene.means3D), opacities=scene.opacities, V=cam.world_view_transform,
               campos=cam.camera_center)
    if variant == "colors":
        g = torch.Generator().manual_seed(3)
        inp["colors_precomp"] = torch.rand(scene.means3D.shape[0], 3, generator=g)
    else:
        inp["shs"] = scene.shs
    if variant == "cov":
        S = covariance3d(scene.scales.double(), scene.rotations.double(), 1.0, None)
        inp["cov3D_precomp"] = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).float()
    else:
        inp["scales"], inp["rotations"] = scene.scales, scene.rotations
    return inp


def fragile_free(state, shape, seed=1):
    """A random upstream gradient of `shape` (..., H, W), zero on the state's fragile pixels"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * (~state["fragile"]).to(torch.float32)
