"""Float64 reference of the 4D Gaussian time slice and the harmonic colour coefficients (include/gsr_slice4d.h, fused_slice4d.py), in
plain torch ops; "Real-time Photorealistic Dynamic Scene Representation and Rendering with 4D Gaussian Splatting" (Yang et al.).

A 4-vector (x, y, z, t) is the quaternion t + x i + y j + z k; with l^ = l / |l| and r^ = r / |r| (both (w, x, y, z)) the rotation is
R v = l^ v conj(r^), in the (x, y, z, t) ordering R = L(l^) M(r^):

    L(a,b,c,d) = [  a -d  c  b ]      M(p,q,r,s) = [  p -s  r -q ]
                 [  d  a -b  c ]                   [  s  p -q -r ]
                 [ -c  b  a  d ]                   [ -r  q  p -s ]
                 [ -b -c -d  a ]                   [  q  r  s  p ]

    s_k = m exp(log-scale_k), Sigma = R diag(s^2) R^T, Sigma_tt = Sigma[3,3], u = Sigma[:3,3], v = u / Sigma_tt, D = time - t
    means3D = xyz + v D,  cov3D = Sigma[:3,:3] - u u^T / Sigma_tt (xx, xy, xz, yy, yz, zz),  g = exp(-D^2 / (2 Sigma_tt))
    opacities = sigmoid(opacity) g where g > cutoff, else +0 (the row is masked)

slice4d() is that sequence in any dtype (float64: the reference, gradients from autograd; float32: the stock sequence a user writes).
slice4d_grads() is the hand-derived chain, checked against autograd on the CPU; with absolute=True every incoming gradient and every
Jacobian factor is replaced by its modulus and every difference by a sum, which gives, per element, the sum of the moduli of the terms
the gradient is formed from: the scale of the GPU tests' bars.
"""
import math
from collections import namedtuple

import torch

LEAVES = ("xyz", "t", "scaling", "scaling_t", "rotation", "rotation_r", "opacity")
COLS = {"xyz": 3, "t": 1, "scaling": 3, "scaling_t": 1, "rotation": 4, "rotation_r": 4, "opacity": 1}
SIX = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
TIME = 0.5          # the time stamp of every scene of make_scene
CUTOFF = 0.05
GPU_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
Slice = namedtuple("Slice", "means3D cov3D opacities velocity g mask sigma11 outer sigma_tt")


def make_scene(P, seed=0, time=TIME):
    """-> dict of the seven float32 leaves: raw quaternions ~ N(0, 1), log-scales ~ N(-2, 0.7), time - t ~ N(0, 0.3), logits ~ N(0, 2)"""
    g = torch.Generator().manual_seed(1000 + seed)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return {"xyz": n(P, 3).float(), "t": (time - 0.3 * n(P, 1)).float(), "scaling": (-2.0 + 0.7 * n(P, 3)).float(),
            "scaling_t": (-2.0 + 0.7 * n(P, 1)).float(), "rotation": n(P, 4).float(), "rotation_r": n(P, 4).float(),
            "opacity": (2.0 * n(P, 1)).float()}


def make_incoming(P, seed=0):
    """-> random dL/dmeans3D (P,3), dL/dcov3D (P,6), dL/dopacities (P,1), dL/dvelocity (P,3), float32"""
    g = torch.Generator().manual_seed(2000 + seed)
    return tuple(torch.randn(P, c, generator=g) for c in (3, 6, 1, 3))


def left_matrix(q):
    a, b, c, d = q.unbind(-1)
    return torch.stack([a, -d, c, b, d, a, -b, c, -c, b, a, d, -b, -c, -d, a], dim=-1).view(-1, 4, 4)


def right_matrix(q):
    p, q_, r, s = q.unbind(-1)
    return torch.stack([p, -s, r, -q_, s, p, -q_, -r, -r, q_, p, -s, q_, r, s, p], dim=-1).view(-1, 4, 4)


def rotation4(rotation, rotation_r):
    """-> R (P,4,4) = L(l^) M(r^)"""
    lh = rotation / rotation.norm(dim=1, keepdim=True)
    rh = rotation_r / rotation_r.norm(dim=1, keepdim=True)
    return left_matrix(lh) @ right_matrix(rh)


def slice4d(leaves, time=TIME, scaling_modifier=1.0, cutoff=CUTOFF, dtype=torch.float64):
    """The time slice in `dtype`, every step a torch op (autograd flows through tensors that require it) -> Slice"""
    x = {k: (v if v.dtype == dtype else v.to(dtype)) for k, v in leaves.items()}
    R = rotation4(x["rotation"], x["rotation_r"])
    s = scaling_modifier * torch.exp(torch.cat((x["scaling"], x["scaling_t"]), dim=1))
    sigma = R @ torch.diag_embed(s * s) @ R.transpose(1, 2)
    sigma_tt = sigma[:, 3, 3:4]
    u = sigma[:, :3, 3]
    sigma11 = sigma[:, :3, :3]
    outer = u[:, :, None] * u[:, None, :] / sigma_tt[:, :, None]
    cov = sigma11 - outer
    vel = u / sigma_tt
    delta = time - x["t"]
    means = x["xyz"] + vel * delta
    g = torch.exp(-0.5 * delta * delta / sigma_tt)
    mask = g <= cutoff
    opac = torch.where(mask, torch.zeros_like(g), torch.sigmoid(x["opacity"]) * g)
    six = lambda m: torch.stack([m[:, i, j] for i, j in SIX], dim=1)
    return Slice(means, six(cov), opac, vel, g, mask[:, 0], six(sigma11), six(outer), sigma_tt)


def ambiguous(sl, cutoff=CUTOFF):
    """rows whose mask decision lies within 2^-40 relative of the cutoff"""
    return ((sl.g - cutoff).abs() <= 2.0 ** -40 * cutoff)[:, 0]


def autograd_grads(leaves, incoming, time=TIME, scaling_modifier=1.0, cutoff=CUTOFF, dtype=torch.float64):
    """-> dict of the seven leaf gradients from autograd through slice4d() in `dtype`; incoming: (g_means, g_cov, g_opac, g_vel), any
    of them None.  Masked rows are zeroed, as the kernels define them (4DGS skips such a Gaussian altogether)."""
    x = {k: v.detach().to(dtype).requires_grad_(True) for k, v in leaves.items()}
    sl = slice4d(x, time, scaling_modifier, cutoff, dtype)
    loss = 0.0
    for out, gin in zip((sl.means3D, sl.cov3D, sl.opacities, sl.velocity), incoming):
        if gin is not None:
            loss = loss + (out * gin.to(dtype)).sum()
    grads = torch.autograd.grad(loss, [x[k] for k in LEAVES], allow_unused=True)
    keep = (~sl.mask)[:, None].to(dtype)
    return {k: (torch.zeros_like(x[k]) if g is None else g * keep) for k, g in zip(LEAVES, grads)}


def slice4d_grads(leaves, incoming, time=TIME, scaling_modifier=1.0, cutoff=CUTOFF, absolute=False):
    """The hand-derived chain in float64 -> dict of the seven leaf gradients.  absolute=True: the per-element sum of the moduli of the
    terms (module docstring)."""
    x = {k: v.detach().double() for k, v in leaves.items()}
    P = x["xyz"].shape[0]
    fix = (lambda v: v.abs()) if absolute else (lambda v: v)
    sub = 1.0 if absolute else -1.0
    zero = lambda c: torch.zeros(P, c, dtype=torch.float64)
    gm, gc, go, gv = (zero(c) if t is None else fix(t.double()) for t, c in zip(incoming, (3, 6, 1, 3)))
    ln, rn = x["rotation"].norm(dim=1, keepdim=True), x["rotation_r"].norm(dim=1, keepdim=True)
    lh, rh = x["rotation"] / ln, x["rotation_r"] / rn
    Lt, Mt = left_matrix(lh), right_matrix(rh)
    Rt = Lt @ Mt
    w = (scaling_modifier * torch.exp(torch.cat((x["scaling"], x["scaling_t"]), dim=1))) ** 2          # (P,4)
    sigma_tt = (Rt[:, 3, :] ** 2 * w).sum(1, keepdim=True)
    u = (Rt[:, :3, :] * Rt[:, 3:4, :] * w[:, None, :]).sum(2)
    delta = time - x["t"]
    g = torch.exp(-0.5 * delta * delta / sigma_tt)
    sig = torch.sigmoid(x["opacity"])
    keep = (g > cutoff).double()
    L, M, R, u, delta, lh_, rh_ = fix(Lt), fix(Mt), fix(Rt), fix(u), fix(delta), fix(lh), fix(rh)
    G = torch.zeros(P, 3, 3, dtype=torch.float64)
    for k, (i, j) in enumerate(SIX):
        if i == j:
            G[:, i, i] = gc[:, k]
        else:
            G[:, i, j] = G[:, j, i] = 0.5 * gc[:, k]
    Gu = (G @ u[:, :, None])[:, :, 0]
    gvt = gv + gm * delta
    through_g = go * sig * g                                                                             # dL/dg times g
    du = (sub * 2.0 * Gu + gvt) / sigma_tt
    dstt = ((u * Gu).sum(1, keepdim=True) + sub * (gvt * u).sum(1, keepdim=True) + through_g * 0.5 * delta * delta) / (sigma_tt * sigma_tt)
    D = torch.zeros(P, 4, 4, dtype=torch.float64)
    D[:, :3, :3] = G
    D[:, :3, 3] = D[:, 3, :3] = 0.5 * du
    D[:, 3, 3] = dstt[:, 0]
    dw = torch.einsum("pab,pak,pbk->pk", D, R, R)
    dscale = 2.0 * w * dw
    GR = 2.0 * (D @ R) * w[:, None, :]
    X = GR @ M.transpose(1, 2)         # dL/dL
    Y = L.transpose(1, 2) @ GR         # dL/dM
    s = -sub                           # the sign of a subtracted entry
    dlh = torch.stack([X[:, 0, 0] + X[:, 1, 1] + X[:, 2, 2] + X[:, 3, 3],
                       X[:, 0, 3] - s * X[:, 1, 2] + X[:, 2, 1] - s * X[:, 3, 0],
                       X[:, 0, 2] + X[:, 1, 3] - s * X[:, 2, 0] - s * X[:, 3, 1],
                       -s * X[:, 0, 1] + X[:, 1, 0] + X[:, 2, 3] - s * X[:, 3, 2]], dim=1)
    drh = torch.stack([Y[:, 0, 0] + Y[:, 1, 1] + Y[:, 2, 2] + Y[:, 3, 3],
                       -s * Y[:, 0, 3] - s * Y[:, 1, 2] + Y[:, 2, 1] + Y[:, 3, 0],
                       Y[:, 0, 2] - s * Y[:, 1, 3] - s * Y[:, 2, 0] + Y[:, 3, 1],
                       -s * Y[:, 0, 1] + Y[:, 1, 0] - s * Y[:, 2, 3] + Y[:, 3, 2]], dim=1)
    dl = (dlh + sub * lh_ * (lh_ * dlh).sum(1, keepdim=True)) / ln
    dr = (drh + sub * rh_ * (rh_ * drh).sum(1, keepdim=True)) / rn
    dt = sub * (gm * u).sum(1, keepdim=True) / sigma_tt + through_g * delta / sigma_tt
    out = {"xyz": gm, "t": dt, "scaling": dscale[:, :3], "scaling_t": dscale[:, 3:], "rotation": dl, "rotation_r": dr,
           "opacity": go * g * sig * (1.0 - sig)}
    return {k: v * keep for k, v in out.items()}


def forward_bars(sl, leaves, time=TIME):
    """-> dict of the forward bars (P, c): 2^-24 |ref| + 2^-40 (the magnitude of the terms the value is formed from)"""
    a, b = 2.0 ** -24, 2.0 ** -40
    xyz, delta = leaves["xyz"].double(), time - leaves["t"].double()
    return {"means3D": a * sl.means3D.abs() + b * (xyz.abs() + (sl.velocity * delta).abs()),
            "cov3D": a * sl.cov3D.abs() + b * (sl.sigma11.abs() + sl.outer.abs()),
            "opacities": a * sl.opacities.abs() + b * sl.opacities.abs(),
            "velocity": a * sl.velocity.abs() + b * sl.velocity.abs()}


# ---- harmonic colour coefficients ----
def make_features(P, N, M, seed=0):
    g = torch.Generator().manual_seed(3000 + seed + 17 * N + 131 * M)
    return torch.randn(P, N + 1, M, 3, generator=g), torch.randn(P, M, 3, generator=g)


def harmonic_coefficients(t, time, period, N):
    """-> c (P, N+1) float64 holding fp32(cos(2 pi n (time - t) / period)), and the unrounded sines"""
    n = torch.arange(N + 1, dtype=torch.float64)[None, :]
    arg = 2.0 * math.pi * n * (time - t.double()) / period
    return torch.cos(arg).float().double(), torch.sin(arg)


def harmonic(features_t, t, time, period):
    """-> shs (P, M, 3) float64 and the bar's scale sum_n |c_n f_n|"""
    N = features_t.shape[1] - 1
    c, _ = harmonic_coefficients(t, time, period, N)
    terms = c[:, :, None, None] * features_t.double()
    return terms.sum(1), terms.abs().sum(1)


def harmonic_grads(features_t, t, time, period, g_shs):
    """-> dfeatures_t (P, N+1, M, 3), dt (P, 1) and sum |terms| of dt (P, 1), float64"""
    N = features_t.shape[1] - 1
    c, s = harmonic_coefficients(t, time, period, N)
    n = torch.arange(N + 1, dtype=torch.float64)[None, :]
    dot = (features_t.double() * g_shs.double()[:, None]).sum((2, 3))
    absdot = (features_t.double() * g_shs.double()[:, None]).abs().sum((2, 3))
    k = 2.0 * math.pi * n / period
    return c[:, :, None, None] * g_shs.double()[:, None], (k * s * dot).sum(1, keepdim=True), (k * s.abs() * absdot).sum(1, keepdim=True)
