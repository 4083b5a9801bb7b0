"""GPU: anti-aliased rendering (GaussianRasterizer(..., antialiasing=True), include/gsr_aa.h): the screen-space filter of
Mip-Splatting, opacity * rho with rho = sqrt(max(2.5e-5, det(Sigma) / det(Sigma + 0.3 I))) over the undilated 2D covariance.

The reference side of the parity checks is the existing rasterizer fed opacities' = o rho + (o_rec - o rho).detach(): rho computed
in float64 torch from the 3D inputs (the clamp conventions of torch_splat.py), o_rec the anti-aliased call's record opacity read
through the published geometry layout.  Its value is bit for bit the fused path's, so every decision of the two runs is the same;
its gradient flows through torch's rho."""
import math

import numpy as np
import pytest
import torch

import gsr_scene
import util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _cov2d64(means3D, st, scales=None, rotations=None, cov3D=None):
    """(a, b, c): the projected covariance BEFORE the 0.3 dilation, float64, differentiable (torch_splat.py's conventions: the
    clamped t.x / t.y held constant, the quaternion unnormalised)."""
    dt = torch.float64
    W, H = int(st.image_width), int(st.image_height)
    V = st.viewmatrix.to(dt)
    fx, fy = W / (2.0 * st.tanfovx), H / (2.0 * st.tanfovy)
    m = means3D.to(dt)
    t = (torch.cat([m, torch.ones_like(m[:, :1])], 1) @ V)[:, :3]
    tz = t[:, 2]
    limx, limy = 1.3 * st.tanfovx, 1.3 * st.tanfovy
    in_x = (t[:, 0] / tz).detach().abs() <= limx
    in_y = (t[:, 1] / tz).detach().abs() <= limy
    tx = torch.where(in_x, t[:, 0], (torch.sign(t[:, 0]) * limx * tz).detach())
    ty = torch.where(in_y, t[:, 1], (torch.sign(t[:, 1]) * limy * tz).detach())
    P = m.shape[0]
    if cov3D is None:
        q = rotations.to(dt)
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                          2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                          2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(P, 3, 3)
        Mm = Rm @ torch.diag_embed(scales.to(dt))
        Sigma = Mm @ Mm.transpose(1, 2)
    else:
        c6 = cov3D.to(dt)
        Sigma = torch.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], 1).reshape(P, 3, 3)
    J = torch.zeros(P, 2, 3, dtype=dt, device=m.device)
    J[:, 0, 0] = fx / tz
    J[:, 0, 2] = -fx * tx / (tz * tz)
    J[:, 1, 1] = fy / tz
    J[:, 1, 2] = -fy * ty / (tz * tz)
    JW = J @ V[:3, :3].t()
    cov = JW @ Sigma @ JW.transpose(1, 2)
    return cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]


def _rho64(a, b, c):
    N = a * c - b * b
    Dh = (a + 0.3) * (c + 0.3) - b * b
    return torch.sqrt(torch.clamp_min(N / Dh, 2.5e-5))


def _safe(x, vis, fill):
    """rows of invisible Gaussians replaced by a harmless constant (no gradient, no inf / nan in the float64 chain)"""
    return torch.where(vis[:, None], x, torch.as_tensor(fill, dtype=x.dtype, device=x.device).expand_as(x))


def _binding_call(st, D, inp, antialiasing, opacities=None, debug=0):
    """-> (num_rendered, color, radii, geom) of one _C.rasterize_gaussians call on detached inputs"""
    from diff_gaussian_rasterization import _C
    e = torch.empty(0, device=DEV)
    g = lambda k: inp[k].detach() if inp.get(k) is not None else e
    R, color, radii, geom, _, _ = _C.rasterize_gaussians(
        st.bg, g("means3D"), g("colors_precomp"), (inp["opacities"] if opacities is None else opacities).detach(), g("scales"),
        g("rotations"), st.scale_modifier, g("cov3D_precomp"), st.viewmatrix, st.projmatrix, st.tanfovx, st.tanfovy,
        st.image_height, st.image_width, g("shs"), D, st.campos, st.prefiltered, debug, antialiasing=antialiasing)
    return R, color, radii, geom


def _record_opacity(geom, P):
    from diff_gaussian_rasterization import _C
    off = _C.geometry_layout(P).splat
    return geom[off: off + 48 * P].view(torch.float32).view(P, 12)[:, 5].clone()


def _inputs(scene, kind):
    t = {"means3D": scene.means3D, "opacities": scene.opacities}
    if "colors" in kind:
        g = torch.Generator().manual_seed(4)
        t["colors_precomp"] = torch.rand(scene.means3D.shape[0], 3, generator=g)
    else:
        t["shs"] = scene.shs
    if "cov3d" in kind:
        a, b, c = _cov3d_of(scene)
        t["cov3D_precomp"] = torch.stack([a[:, 0, 0], a[:, 0, 1], a[:, 0, 2], a[:, 1, 1], a[:, 1, 2], a[:, 2, 2]], 1)
    else:
        t["scales"], t["rotations"] = scene.scales, scene.rotations
    return {k: v.to(DEV).contiguous().clone().requires_grad_(True) for k, v in t.items()}


def _cov3d_of(scene):
    q = scene.rotations.double()
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    P = q.shape[0]
    Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                      2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                      2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(P, 3, 3)
    Mm = Rm @ torch.diag_embed(scene.scales.double())
    return (Mm @ Mm.transpose(1, 2)).float(), None, None


def _grads(t):
    return {k: (v.grad.clone() if v.grad is not None else torch.zeros_like(v)) for k, v in t.items()}


def fused(scene, cam, D, kind, dpix, mode=None, dD=None, dA=None, debug=0, antialiasing=True):
    from diff_gaussian_rasterization import GaussianRasterizer
    st = util.hip_settings(scene, cam, D, DEV, debug=debug)
    t = _inputs(scene, kind)
    m2 = torch.zeros_like(t["means3D"], requires_grad=True)
    out = GaussianRasterizer(st, depth_alpha=mode, antialiasing=antialiasing)(means2D=m2, **t)
    loss = (out[0] * dpix).sum()
    if dD is not None:
        loss = loss + (out[2] * dD).sum()
    if dA is not None:
        loss = loss + (out[3] * dA).sum()
    loss.backward()
    torch.cuda.synchronize()
    g = _grads(t)
    g["means2D"] = m2.grad.clone()
    return [o.detach() for o in out], g


def composed(scene, cam, D, kind, dpix, mode=None, dD=None, dA=None, split=False):
    """The reference composition -> (outputs, grads, o_rec, radii_default, R_aa, R_ref, t)"""
    from diff_gaussian_rasterization import GaussianRasterizer
    st = util.hip_settings(scene, cam, D, DEV)
    t = _inputs(scene, kind)
    P = t["means3D"].shape[0]
    R_aa, _, radii_aa, geom = _binding_call(st, D, t, True)
    R_def, _, radii_def, _ = _binding_call(st, D, t, False)
    assert torch.equal(radii_aa, radii_def)
    o_rec = _record_opacity(geom, P)
    vis = radii_aa > 0
    a, b, c = _cov2d64(_safe(t["means3D"], vis, [0.0, 0.0, 5.0]), st,
                       scales=None if "cov3D_precomp" in t else _safe(t["scales"], vis, [0.01, 0.01, 0.01]),
                       rotations=None if "cov3D_precomp" in t else _safe(t["rotations"], vis, [1.0, 0.0, 0.0, 0.0]),
                       cov3D=_safe(t["cov3D_precomp"], vis, [1e-4, 0, 0, 1e-4, 0, 1e-4]) if "cov3D_precomp" in t else None)
    rho = _rho64(a, b, c)
    o64 = t["opacities"].double() * rho[:, None]
    op = torch.where(vis[:, None], o64 + (o_rec.double()[:, None] - o64).detach(), t["opacities"].double()).float()
    assert torch.equal(op[vis, 0], o_rec[vis])
    R_ref, _, _, _ = _binding_call(st, D, t, False, opacities=op)
    m2 = torch.zeros_like(t["means3D"], requires_grad=True)
    inp = dict(t)
    inp["opacities"] = op
    out = GaussianRasterizer(st, depth_alpha=mode)(means2D=m2, **inp)
    if split:
        part = torch.randn(dpix.shape, generator=torch.Generator().manual_seed(99)).to(DEV)
        out2 = GaussianRasterizer(st, depth_alpha=mode)(means2D=m2, **inp)
        loss = (out[0] * part).sum() + (out2[0] * (dpix - part)).sum()
    else:
        loss = (out[0] * dpix).sum()
    if dD is not None:
        loss = loss + (out[2] * dD).sum()
    if dA is not None:
        loss = loss + (out[3] * dA).sum()
    loss.backward()
    torch.cuda.synchronize()
    g = _grads(t)
    g["means2D"] = m2.grad.clone()
    # the record against a float64 evaluation of o * rho: 2e-6 of o, plus what the fp32 projection's rounding of a, b, c (a few
    # eps32 each) does to N = a c - b^2 where it cancels -- d rho / rho = dN / (2 N), dN ~ 8 eps32 (a c + b^2)
    o_ex = (t["opacities"].detach().double()[:, 0] * rho.detach())[vis]
    a, b, c = a.detach()[vis], b.detach()[vis], c.detach()[vis]
    N = a * c - b * b
    cond = torch.where(rho.detach()[vis] > 0.005, 8 * 2.0 ** -23 * (a * c + b * b) / (2 * N.abs()), torch.zeros_like(N))
    err = (o_rec[vis].double() - o_ex).abs() / t["opacities"].detach().double()[vis, 0]
    print(f"record opacity: max rel err {float(err.max()):.2e}, max over bar {float((err / (2e-6 + cond)).max()):.2f}")
    rel = float((err / (2e-6 + cond)).max()) * 2e-6
    return [o.detach() for o in out], g, rel, radii_def, R_aa, R_ref


def _nerr(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-30)


CHAIN = ("means3D", "scales", "rotations", "cov3D_precomp")


def check_grads(g, rg, band, label):
    """1e-5 of the largest element (test_parity_gpu.py's bar); for the gradients that dL/drho reaches through the covariance chain,
    the reference composition's own reproducibility band as in test_depth_alpha_gpu.py: max(5e-5, 10 x one split-pass sample)."""
    for n in rg:
        e = _nerr(g[n], rg[n])
        b = max(5e-5, 10.0 * _nerr(band[n], rg[n])) if n in CHAIN else 1e-5
        print(f"{label} {n}: {e:.2e} (bar {b:.2e})")
        assert e <= b, (label, n, e, b)


def _c1():
    return gsr_scene.make_scene(10_000, -3.5, sh_degree=3, seed=5), gsr_scene.make_camera(256, 256), 3


def _heavy():
    from test_boundary_gpu import _heavy_scene
    return _heavy_scene()


CASES = {"C1": _c1, "C2": lambda: gsr_scene.make_config("C2", seed=2), "C3": lambda: gsr_scene.make_config("C3", seed=3),
         "heavy": _heavy}


def _dpix(seed, H, W):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(3, H, W, generator=g).to(DEV), torch.randn(1, H, W, generator=g).to(DEV),
            torch.randn(1, H, W, generator=g).to(DEV))


def _check(scene, cam, D, kind, label, mode=None, use_maps=False, seed=1):
    H, W = cam.image_height, cam.image_width
    dpix, dD, dA = _dpix(seed, H, W)
    if not use_maps:
        dD = dA = None
    f, g = fused(scene, cam, D, kind, dpix, mode, dD, dA)
    r, rg, rel, radii_def, R_aa, R_ref = composed(scene, cam, D, kind, dpix, mode, dD, dA)
    _, band, _, _, _, _ = composed(scene, cam, D, kind, dpix, mode, dD, dA, split=True)
    assert R_aa == R_ref, (R_aa, R_ref)
    assert torch.equal(f[0], r[0]), label
    assert torch.equal(f[1], radii_def), label
    if mode is not None:
        assert torch.equal(f[2], r[2]) and torch.equal(f[3], r[3]), label
    assert rel <= 2e-6, (label, rel)
    check_grads(g, rg, band, label)


@pytest.mark.parametrize("case", list(CASES))
def test_composition_parity(case):
    scene, cam, D = CASES[case]()
    _check(scene, cam, D, "sh", case)


@pytest.mark.parametrize("kind", ["colors", "cov3d", "colors_cov3d"])
def test_composition_parity_precomputed_inputs(kind):
    scene, cam, D = _c1()
    _check(scene, cam, D, kind, kind, seed=2)


@pytest.mark.parametrize("mode", ["depth", "invdepth"])
@pytest.mark.parametrize("use_maps", [False, True])
def test_composition_parity_with_depth_alpha(mode, use_maps):
    scene, cam, D = gsr_scene.make_config("C2", seed=2)
    _check(scene, cam, D, "sh", f"{mode}/{use_maps}", mode=mode, use_maps=use_maps, seed=3)


def _leaf_params(scene):
    dc = scene.shs[:, :1, :].contiguous()
    rest = scene.shs[:, 1:, :].contiguous()
    g = torch.Generator().manual_seed(3)
    raw_rot = scene.rotations * (0.5 + torch.rand(scene.rotations.shape[0], 1, generator=g))
    return {"xyz": scene.means3D, "features_dc": dc, "features_rest": rest, "opacity": torch.logit(scene.opacities),
            "scaling": torch.log(scene.scales), "rotation": raw_rot}


@pytest.mark.parametrize("mode", [None, "depth"])
def test_leaf_parameters(mode):
    """rasterize_leaf_gaussians(antialiasing=True) against GaussianRasterizer(antialiasing=True) fed the activations computed in torch:
    the logit gradient carries the sigmoid backward of dL/dopacity_in."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from fused_params import rasterize_leaf_gaussians
    scene, cam, D = _heavy()
    H, W = cam.image_height, cam.image_width
    dpix, dD, dA = _dpix(15, H, W)
    lp = _leaf_params(scene)
    st = util.hip_settings(scene, cam, D, DEV)

    def leaves():
        return {k: v.to(DEV).clone().requires_grad_(True) for k, v in lp.items()}

    def run(split_part=None):
        t = leaves()
        m2 = torch.zeros_like(t["xyz"], requires_grad=True)
        out = rasterize_leaf_gaussians(t["xyz"], m2, t["features_dc"], t["features_rest"], t["opacity"], t["scaling"], t["rotation"], st,
                                       depth_alpha=mode, antialiasing=True)
        loss = (out[0] * dpix).sum() + ((out[2] * dD).sum() + (out[3] * dA).sum() if mode else 0.0)
        loss.backward()
        torch.cuda.synchronize()
        return [o.detach() for o in out], {**_grads(t), "means2D": m2.grad.clone()}

    def ref(split=False):
        t = leaves()
        m2 = torch.zeros_like(t["xyz"], requires_grad=True)
        sh = torch.cat([t["features_dc"], t["features_rest"]], 1)
        rot = torch.nn.functional.normalize(t["rotation"])
        out = GaussianRasterizer(st, depth_alpha=mode, antialiasing=True)(
            means3D=t["xyz"], means2D=m2, shs=sh, opacities=torch.sigmoid(t["opacity"]), scales=torch.exp(t["scaling"]), rotations=rot)
        if split:
            part = torch.randn(dpix.shape, generator=torch.Generator().manual_seed(99)).to(DEV)
            out2 = GaussianRasterizer(st, depth_alpha=mode, antialiasing=True)(
                means3D=t["xyz"], means2D=m2, shs=sh, opacities=torch.sigmoid(t["opacity"]), scales=torch.exp(t["scaling"]),
                rotations=rot)
            loss = (out[0] * part).sum() + (out2[0] * (dpix - part)).sum()
        else:
            loss = (out[0] * dpix).sum()
        loss = loss + ((out[2] * dD).sum() + (out[3] * dA).sum() if mode else 0.0)
        loss.backward()
        torch.cuda.synchronize()
        return [o.detach() for o in out], {**_grads(t), "means2D": m2.grad.clone()}

    f, g = run()
    r, rg = ref()
    _, band = ref(split=True)
    assert torch.equal(f[1], r[1])
    for k in range(len(f)):
        if k != 1:
            assert _nerr(f[k], r[k]) <= 1e-6, k
    for n in rg:
        e = _nerr(g[n], rg[n])
        b = max(5e-5, 10.0 * _nerr(band[n], rg[n])) if n in ("xyz", "scaling", "rotation") else 2e-5
        print(f"leaf/{mode} {n}: {e:.2e} (bar {b:.2e})")
        assert e <= b, (n, e, b)
    assert float(g["opacity"].abs().max()) > 0


def test_oracle_pin():
    """The image against the CPU oracle fed opacities = o rho (rho in float64 from the 3D inputs)."""
    scene, cam, D = gsr_scene.make_scene(3_000, -3.0, sh_degree=1, seed=21), gsr_scene.make_camera(120, 90), 1
    st = util.hip_settings(scene, cam, D, DEV)
    t = _inputs(scene, "sh")
    _, color, radii, _ = _binding_call(st, D, t, True)
    vis = radii > 0
    a, b, c = _cov2d64(_safe(t["means3D"].detach(), vis, [0.0, 0.0, 5.0]), st, scales=_safe(t["scales"].detach(), vis, [0.01] * 3),
                       rotations=_safe(t["rotations"].detach(), vis, [1.0, 0.0, 0.0, 0.0]))
    op = (scene.opacities.double() * _rho64(a, b, c).cpu()[:, None]).float()
    o = util.oracle_forward(scene._replace(opacities=op.contiguous()), cam, D)
    ok = o["fragile"].reshape(cam.image_height, cam.image_width) == 0
    assert ok.mean() > 0.9
    assert np.abs(color.cpu().numpy() - o["color"])[:, ok].max() <= 1e-5
    assert np.array_equal(radii.cpu().numpy(), o["radii"])


# one isolated sub-pixel Gaussian (camera at (0, 0, -4) looking down +z; the Gaussian at z = 0, 4 units in front)
_SIGMAS = {"iso": (0.09, 0.0, 0.09), "aniso": (0.16, 0.02, 0.04), "skew": (0.25, -0.05, 0.03)}
_OFFSETS = [(0.0, 0.0), (0.25, 0.1), (0.5, 0.5), (-0.3, 0.4)]


@pytest.mark.parametrize("shape", list(_SIGMAS))
def test_subpixel_gaussian_keeps_its_footprint(shape):
    """What the filter is for: with it, the pixel sum of alpha is the footprint integral o 2 pi sqrt(det Sigma) of the undilated
    Gaussian (to 5 %, the 1/255 cut integrated the same way); without it, that times sqrt(Dh / N) -- 4.3x for the isotropic 0.3 px."""
    from diff_gaussian_rasterization import GaussianRasterizer
    W = H = 48
    cam = gsr_scene.make_camera(W, H)
    scene = gsr_scene.make_scene(1, -3.0, sh_degree=0, seed=1)._replace(bg=torch.zeros(3))
    st = util.hip_settings(scene, cam, 0, DEV)
    fx, fy = W / (2.0 * st.tanfovx), H / (2.0 * st.tanfovy)
    a2, b2, c2 = _SIGMAS[shape]
    z = 4.0
    for dx, dy in _OFFSETS:
        mean = torch.tensor([[dx * z / fx, dy * z / fy, 0.0]])
        # 3D covariance whose projection at the image centre is the wanted Sigma (J = diag(fx, fy) / z there; a thin z extent)
        cov = torch.tensor([[a2 * (z / fx) ** 2, b2 * z * z / (fx * fy), 0.0, c2 * (z / fy) ** 2, 0.0, 1e-8]])
        o = torch.tensor([[0.99]])
        args = dict(means3D=mean.to(DEV), means2D=torch.zeros(1, 3, device=DEV), opacities=o.to(DEV),
                    colors_precomp=torch.ones(1, 3, device=DEV), cov3D_precomp=cov.to(DEV))
        img_aa, _ = GaussianRasterizer(st, antialiasing=True)(**args)
        img, _ = GaussianRasterizer(st)(**args)
        s_aa, s_def = float(img_aa[0].double().sum()), float(img[0].double().sum())
        # expectation: the same blend of the same splat in float64 over the pixel centres, alpha < 1/255 cut, clamp at 0.99
        a, b, c = (float(v) for v in _cov2d64(mean.to(DEV), st, cov3D=cov.to(DEV)))
        N, Dh = a * c - b * b, (a + 0.3) * (c + 0.3) - b * b
        rho = math.sqrt(max(2.5e-5, N / Dh))
        hom = torch.cat([mean.double(), torch.ones(1, 1, dtype=torch.float64)], 1) @ st.projmatrix.double().cpu()
        px = ((hom[0, 0] / hom[0, 3] + 1.0) * W - 1.0) * 0.5
        py = ((hom[0, 1] / hom[0, 3] + 1.0) * H - 1.0) * 0.5
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        ddx, ddy = px - xs, py - ys
        ca, cb, cc = (c + 0.3) / Dh, -b / Dh, (a + 0.3) / Dh
        g = torch.exp(-0.5 * (ca * ddx * ddx + cc * ddy * ddy) - cb * ddx * ddy)

        def blend(op):
            al = torch.clamp_max(op * g, 0.99)
            return float(torch.where(al >= 1.0 / 255.0, al, torch.zeros_like(al)).sum())
        e_aa, e_def = blend(0.99 * rho), blend(0.99)
        footprint = 0.99 * 2.0 * math.pi * math.sqrt(N)
        print(f"{shape} {dx},{dy}: aa {s_aa:.4f} (expected {e_aa:.4f}, footprint {footprint:.4f}); default {s_def:.4f} ({e_def:.4f})")
        assert abs(s_aa - e_aa) <= 0.05 * e_aa
        assert abs(e_aa - footprint) <= 0.05 * footprint   # the cut removes little once compensated
        assert abs(s_def - e_def) <= 0.05 * e_def
        ratio = s_def / s_aa
        assert abs(ratio - math.sqrt(Dh / N)) <= 0.1 * math.sqrt(Dh / N), (ratio, math.sqrt(Dh / N))
        if shape == "iso":
            assert 3.9 < ratio < 4.7


def test_off_is_the_default_path():
    """antialiasing=False is bit-identical to a call without the keyword: image, radii, every gradient, the densification
    statistics."""
    from diff_gaussian_rasterization import GaussianRasterizer
    scene, cam, D = gsr_scene.make_config("C2", seed=2)
    st = util.hip_settings(scene, cam, D, DEV)
    dpix = _dpix(5, cam.image_height, cam.image_width)[0]
    P = scene.means3D.shape[0]

    def run(**kw):
        t = _inputs(scene, "sh")
        m2 = torch.zeros_like(t["means3D"], requires_grad=True)
        stats = tuple(torch.zeros(P, device=DEV) for _ in range(3))
        color, radii = GaussianRasterizer(st, densify_stats=stats, **kw)(means2D=m2, **t)
        (color * dpix).sum().backward()
        torch.cuda.synchronize()
        return color.detach(), radii, {**_grads(t), "means2D": m2.grad.clone()}, stats
    a, b, c = run(), run(antialiasing=False), run(antialiasing=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n
    for x, y in zip(a[3], b[3]):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], c[0])   # and the filter does change the image
    assert torch.equal(a[1], c[1])


@pytest.mark.parametrize("bit", ["DEBUG_NO_TRIM", "DEBUG_NO_SPLIT", "DEBUG_TILE_SORT", "DEBUG_RADIX_DEPTH"])
def test_debug_bits_and_determinism(bit):
    """The anti-aliased outputs are bit-identical under the diagnostic bits and from run to run (as the default path's are; the
    backward's split / unsplit tile segments sum in other orders, so there the gradients agree to rounding as in
    test_depth_alpha_gpu.py)."""
    from diff_gaussian_rasterization import _C
    scene, cam, D = _heavy()
    dpix = _dpix(18, cam.image_height, cam.image_width)[0]
    a = fused(scene, cam, D, "sh", dpix)
    a2 = fused(scene, cam, D, "sh", dpix)
    b = fused(scene, cam, D, "sh", dpix, debug=getattr(_C, bit))
    for x, y in ((a, a2), (a, b)):
        assert torch.equal(x[0][0], y[0][0]) and torch.equal(x[0][1], y[0][1])
    for n in a[1]:
        assert torch.equal(a[1][n], a2[1][n]), n
    if bit == "DEBUG_RADIX_DEPTH":
        for n in a[1]:
            assert torch.equal(a[1][n], b[1][n]), n
    else:
        for n in a[1]:
            m = float(a[1][n].abs().max())
            tol = 5e-5 if n in CHAIN else 2e-6
            assert float((a[1][n] - b[1][n]).abs().max()) <= tol * max(m, 1e-30), n


def test_view_parallel_single_rank():
    """rasterize_view_parallel(..., antialiasing=True) with one rank equals GaussianRasterizer(antialiasing=True) bit for bit."""
    import view_parallel
    from diff_gaussian_rasterization import GaussianRasterizer
    P = 7013
    scene = gsr_scene.make_scene(P, -3.0, sh_degree=3, seed=77)
    cam = gsr_scene.ring_camera(240, 136, 2, 8)
    st = util.hip_settings(scene, cam, 3, DEV)
    dpix = torch.randn(3, 136, 240, generator=torch.Generator().manual_seed(3)).to(DEV)
    names = ("means3D", "shs", "opacities", "scales", "rotations")

    def leaves():
        return {k: getattr(scene, k).to(DEV).clone().requires_grad_(True) for k in names}
    p = leaves()
    m2 = torch.zeros_like(p["means3D"], requires_grad=True)
    color, radii = GaussianRasterizer(st, antialiasing=True)(means2D=m2, **p)
    color.backward(dpix)
    ex = view_parallel.GradientExchange(P, 16, DEV, parts=2)
    q = leaves()
    n2 = torch.zeros_like(q["means3D"], requires_grad=True)
    color2, radii2 = view_parallel.rasterize_view_parallel(q["means3D"], n2, q["shs"], q["opacities"], q["scales"], q["rotations"], st, ex,
                                                           antialiasing=True)
    color2.backward(dpix)
    assert torch.equal(color, color2) and torch.equal(radii, radii2)
    assert torch.equal(m2.grad, n2.grad)
    for k in names:
        assert torch.equal(p[k].grad, q[k].grad), k
