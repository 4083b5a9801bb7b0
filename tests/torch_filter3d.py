"""Float64 reference of Mip-Splatting's 3D smoothing filter (include/gsr_filter3d.h, fused_filter3d.py) in plain torch, restated from
the published formulas, and the stock sequences a user writes (the per-camera loop with distance[valid] = min(...), prod and
sqrt(det1 / det2), the reset through inverse_sigmoid) in a dtype of the caller's choice.  Also the test scenes, so that the CPU test
that caps the ambiguous rows and the GPU test that skips them look at the same points and cameras."""
import math
from types import SimpleNamespace

import torch

ROOT02 = float(torch.tensor(0.2 ** 0.5, dtype=torch.float32))   # fp32(sqrt(0.2)), the constant the stock fp32 product uses
UNSEEN = 100000.0
U = 2.0 ** -24
# (P, C) of the sweep tests: a lone lane, a wave that is not full, a full wave, a wave and a lane, one below / at / one above the
# workgroup of 256, several workgroups with a remainder
SWEEP_CASES = ((1, 1), (63, 2), (64, 1), (65, 3), (255, 2), (256, 2), (257, 3), (4099, 17))


def ring_cameras(C, radius=4.0, W=64, H=48):
    """C cameras on a ring of `radius` around the y axis, looking at the origin, W x H pixels, focal 50 (1 + 0.1 c) -> camera objects with
    the fields pack_cameras() reads (world_view_transform in the transposed convention: p = x @ wvt[:3,:3] + wvt[3,:3])"""
    cams = []
    for c in range(C):
        th = 2.0 * math.pi * c / C + 0.1
        pos = torch.tensor([radius * math.cos(th), 0.0, radius * math.sin(th)], dtype=torch.float64)
        zax = -pos / pos.norm()
        xax = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), zax)
        xax = xax / xax.norm()
        yax = torch.linalg.cross(zax, xax)
        R = torch.stack([xax, yax, zax])           # world to camera
        wvt = torch.eye(4, dtype=torch.float64)
        wvt[:3, :3] = R.T
        wvt[3, :3] = -R @ pos
        f = 50.0 * (1.0 + 0.1 * c)
        cams.append(SimpleNamespace(world_view_transform=wvt.float(), FoVx=2.0 * math.atan(W / (2.0 * f)), FoVy=2.0 * math.atan(H / (2.0 * f)),
                                    image_width=W, image_height=H))
    return cams


def sweep_scene(P, C):
    """-> (xyz (P,3) float32 uniform in [-3, 3]^3, the C ring cameras); the seed is a function of the case"""
    g = torch.Generator().manual_seed(1000 * P + C)
    return 6.0 * torch.rand(P, 3, generator=g) - 3.0, ring_cameras(C)


def unseen_scene(P=70):
    """every point lies behind the one camera: no row is valid"""
    g = torch.Generator().manual_seed(P)
    xyz = 6.0 * torch.rand(P, 3, generator=g) - 3.0
    cams = ring_cameras(1)
    pos = -cams[0].world_view_transform[:3, :3].double() @ cams[0].world_view_transform[3, :3].double()
    return (xyz.double() + 2.5 * pos).float(), cams


def _project(xyz, rec):
    """xyz (P,3), rec (C,20) packed records -> p (C,P,3), pixel x and y (C,P), all float64, and the records' columns as (C,1)"""
    x = xyz.double()
    r = rec.double()
    R, t = r[:, :9].reshape(-1, 3, 3), r[:, 9:12]
    p = torch.einsum("cjk,pk->cpj", R, x) + t[:, None, :]
    fx, fy, cx, cy, W, H = (r[:, 12 + k][:, None] for k in range(6))
    return p, p[..., 0] / p[..., 2] * fx + cx, p[..., 1] / p[..., 2] * fy + cy, (R, t, fx, fy, cx, cy, W, H)


def sweep(xyz, rec, per_camera=False):
    """The float64 reference of gsr_filter3d_compute on packed float32 records -> a namespace: filter (P,), seen (P,) bool, winner (P,)
    the camera that sets d, zsum (P,) = sum_k |R_2k x_k| + |t_2| at the winner, focal (P,) = f_max or the winner's fx, ambiguous (P,)
    bool, dmax_row (the row holding the largest d, or -1), risky: an ambiguous decision whose d would exceed the largest valid one."""
    p, px, py, (R, t, fx, fy, cx, cy, W, H) = _project(xyz, rec)
    z = p[..., 2]
    valid = (z > 0.2) & (px >= -0.15 * W) & (px <= 1.15 * W) & (py >= -0.15 * H) & (py <= 1.15 * H)
    cand = z / fx if per_camera else z
    big = torch.full_like(cand, float("inf"))
    d, winner = torch.where(valid, cand, big).min(dim=0)
    seen = valid.any(dim=0)
    fmax = float(rec[:, 12].double().max())
    # what a decision's own fp32 inputs leave open
    ax = xyz.double().abs()
    rows = torch.einsum("cjk,pk->cpj", R.abs(), ax)                       # sum_k |R_jk x_k|
    zsum_all = rows[..., 2] + t[:, 2].abs()[:, None]
    near_z = (z - 0.2).abs() <= 16 * U * zsum_all
    zc = z.clamp(min=0.1)
    mx = 32 * U * (rows[..., 0] * fx / zc + px.abs() + W)
    my = 32 * U * (rows[..., 1] * fy / zc + py.abs() + H)
    near_px = ((px + 0.15 * W).abs() <= mx) | ((px - 1.15 * W).abs() <= mx) | ((py + 0.15 * H).abs() <= my) | ((py - 1.15 * H).abs() <= my)
    open_ = near_z | ((z > 0.2) & near_px)
    ambiguous = open_.any(dim=0)
    out = SimpleNamespace(seen=seen, winner=winner, ambiguous=ambiguous, fmax=fmax)
    if bool(seen.any()):
        dmax, out.dmax_row = float(d[seen].max()), int(torch.where(seen, d, -big[0]).argmax())
        d = torch.where(seen, d, torch.full_like(d, dmax))
        winner = torch.where(seen, winner, winner[out.dmax_row])
        out.filter = d * ROOT02 if per_camera else d / fmax * ROOT02
        out.risky = bool((open_ & (cand > dmax)).any())
    else:
        out.dmax_row, out.risky = -1, False
        out.filter = torch.full_like(d, UNSEEN)
    idx = torch.arange(xyz.shape[0])
    out.zsum = zsum_all[winner, idx]
    out.focal = fx[winner, 0] if per_camera else torch.full_like(d, fmax)
    out.d = d
    return out


def sweep_bound(ref):
    """The GPU sweep's error bar per row: the three-term dot product with its translation, with room for contraction, carried through
    1 / f; then one division, one product and the rounded constant (2.5 * 2^-24 relative in all, 4 allowed)."""
    return ROOT02 * 16 * U * ref.zsum / ref.focal + 4 * U * ref.filter


def stock_sweep(xyz, cams, per_camera=False, dtype=torch.float64):
    """Mip-Splatting's compute_3D_filter as published: the loop over the cameras (centred principal point), in `dtype`"""
    x = xyz.to(dtype)
    distance = torch.ones(x.shape[0], dtype=dtype) * 100000.0
    valid_points = torch.zeros(x.shape[0], dtype=torch.bool)
    focal_length = 0.0
    for cam in cams:
        W, H = cam.image_width, cam.image_height
        fx, fy = W / (2.0 * math.tan(0.5 * cam.FoVx)), H / (2.0 * math.tan(0.5 * cam.FoVy))
        if dtype == torch.float64:   # the records carry float32 intrinsics: the comparison to 1e-12 is about the sequence, not about them
            fx, fy = float(torch.tensor(fx, dtype=torch.float32)), float(torch.tensor(fy, dtype=torch.float32))
        wvt = cam.world_view_transform.to(dtype)
        xyz_cam = x @ wvt[:3, :3] + wvt[3, :3][None, :]
        z = xyz_cam[:, 2]
        in_front = z > 0.2
        u = xyz_cam[:, 0] / torch.clamp(z, min=0.001) * fx + W / 2.0
        v = xyz_cam[:, 1] / torch.clamp(z, min=0.001) * fy + H / 2.0
        in_screen = torch.logical_and(torch.logical_and(u >= -0.15 * W, u <= W * 1.15), torch.logical_and(v >= -0.15 * H, v <= 1.15 * H))
        valid = torch.logical_and(in_front, in_screen)
        cand = z / fx if per_camera else z
        distance[valid] = torch.min(distance[valid], cand[valid])
        valid_points = torch.logical_or(valid_points, valid)
        focal_length = max(focal_length, fx)
    distance[~valid_points] = distance[valid_points].max()
    return (distance * (0.2 ** 0.5) if per_camera else distance / focal_length * (0.2 ** 0.5))[:, None]


# ---- activations ----
def make_leaves(P, seed, ls_range=(-9.0, 2.0), logit_range=8.0, f_range=(1e-4, 1e-1)):
    """-> (logits (P,1), log-scales (P,3), filter (P,1)) float32; the filter is log-uniform"""
    g = torch.Generator().manual_seed(seed)
    opacity = (2.0 * torch.rand(P, 1, generator=g) - 1.0) * logit_range
    scaling = ls_range[0] + (ls_range[1] - ls_range[0]) * torch.rand(P, 3, generator=g)
    lo, hi = math.log(f_range[0]), math.log(f_range[1])
    return opacity, scaling, torch.exp(lo + (hi - lo) * torch.rand(P, 1, generator=g))


def activations(opacity, scaling, filter_3d):
    """-> (opacities (P,1), scales (P,3), coef (P,1)) in float64, the coefficient per axis"""
    l, s, f = opacity.double(), torch.exp(scaling.double()), filter_3d.double()
    root = torch.sqrt(s * s + f * f)
    coef = (s / root).prod(dim=1, keepdim=True)
    return torch.sigmoid(l) * coef, root, coef


def activation_grads(opacity, scaling, filter_3d, g_o, g_s):
    """-> (dL/dl (P,1), term1 (P,3), term2 (P,3)) in float64 with dL/dls = term1 + term2; g_o (P,1) and g_s (P,3), None = zero"""
    l, s, f = opacity.double(), torch.exp(scaling.double()), filter_3d.double()
    a, ff = s * s, f * f
    b = a + ff
    opac, _, coef = activations(opacity, scaling, filter_3d)
    go = torch.zeros_like(l) if g_o is None else g_o.double()
    gs = torch.zeros_like(s) if g_s is None else g_s.double()
    return go * torch.sigmoid(l) * torch.sigmoid(-l) * coef, gs * a / torch.sqrt(b), go * opac * ff / b


def stock_activations(opacity, scaling, filter_3d, dtype=torch.float32):
    """get_opacity_with_3D_filter and get_scaling_with_3D_filter as published, in `dtype`; autograd flows into opacity and scaling
    where they are leaves of that dtype"""
    l = opacity if opacity.dtype == dtype else opacity.to(dtype)
    ls = scaling if scaling.dtype == dtype else scaling.to(dtype)
    f = filter_3d.to(dtype)
    scales = torch.exp(ls)
    scales_square = torch.square(scales)
    det1 = scales_square.prod(dim=1)
    scales_after_square = scales_square + torch.square(f)
    det2 = scales_after_square.prod(dim=1)
    coef = torch.sqrt(det1 / det2)
    return torch.sigmoid(l) * coef[..., None], torch.sqrt(scales_after_square)


def reset_logits(opacity, scaling, filter_3d, max_opacity=0.01):
    """-> (new logits (P,1) float64, changed (P,1) bool): logit(min(sigmoid(l), max_opacity / coef)), a row at or below the cap keeps
    its logit"""
    l = opacity.double()
    _, _, coef = activations(opacity, scaling, filter_3d)
    cap = max_opacity / coef
    changed = torch.sigmoid(l) > cap
    capc = torch.where(changed, cap, torch.full_like(cap, 0.5))
    return torch.where(changed, torch.log(capc) - torch.log1p(-capc), l), changed


def stock_reset_logits(opacity, scaling, filter_3d, max_opacity=0.01, dtype=torch.float64):
    """Mip-Splatting's reset_opacity as published: min on the filtered opacity, the coefficient divided out, inverse_sigmoid"""
    opac, _ = stock_activations(opacity.to(dtype), scaling.to(dtype), filter_3d, dtype)
    l, ls, f = opacity.to(dtype), scaling.to(dtype), filter_3d.to(dtype)
    opacities_new = torch.min(opac, torch.ones_like(opac) * max_opacity)
    scales_square = torch.square(torch.exp(ls))
    coef = torch.sqrt(scales_square.prod(dim=1) / (scales_square + torch.square(f)).prod(dim=1))
    x = opacities_new / coef[..., None]
    return torch.log(x / (1 - x))


def baked(opacity, scaling, filter_3d):
    """-> (logit(opacities) (P,1), log(scales) (P,3)) in float64; 1 - opacities as sigmoid(-l) + sigmoid(l) (1 - coef)"""
    l = opacity.double()
    opac, root, coef = activations(opacity, scaling, filter_3d)
    return torch.log(opac) - torch.log(torch.sigmoid(-l) + torch.sigmoid(l) * (1.0 - coef)), torch.log(root)


def ulps(got, want64):
    """the distance of float32 `got` from float64 `want64` rounded to float32, in units of the last place of the rounded value"""
    w = want64.float()
    a, b = got.contiguous().view(torch.int32).long(), w.contiguous().view(torch.int32).long()
    flip = lambda v: torch.where(v < 0, -(v & 0x7FFFFFFF), v)   # sign-magnitude to a monotone integer line
    return (flip(a) - flip(b)).abs()
