"""GPU: the per-Gaussian normals, the depth normals, the fused normal-consistency loss (include/gsr_normals.h, fused_geometry.py) and
render(normals=True), against the float64 restatement of tests/torch_normals.py.

The bar is tests/test_loss.py's: maps within 1e-5 absolute, gradients within 1e-5 of the largest reference gradient.  Where the same
formula evaluated by torch in fp32 (the restatement with dtype=float32) is further from float64 than that, the bar is three times
that distance, measured here and printed."""
import math

import pytest
import torch

import torch_normals as tn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TANX = math.tan(0.5)


def _bar(ref64, same32, grad):
    """(bar, distance of fp32 torch from float64) for a map (grad=False) or a gradient (grad=True)"""
    base = 1e-5 * (float(ref64.abs().max()) if grad else 1.0)
    d32 = float((same32.double() - ref64).abs().max())
    return (base if d32 <= base else 3.0 * d32), d32


def _check(what, got, ref64, same32, grad):
    bar, d32 = _bar(ref64, same32, grad)
    err = float((got.double().cpu() - ref64).abs().max())
    print(f"{what}: err {err:.3e} bar {bar:.3e} (fp32 torch {d32:.3e}, max |ref| {float(ref64.abs().max()):.3e})")
    assert math.isfinite(err) and err <= bar, (what, err, bar)


# ---- the per-Gaussian kernel -----------------------------------------------------------------------------------------------------------
def _gaussian_case(P, seed=5):
    """fp32 CPU inputs: each axis the smallest in turn, exact ties between two scales and between all three, one zero and one
    unnormalised quaternion, and no facing decision within rounding: |n . t| / |t| >= 0.05 for every Gaussian that has a normal."""
    import gsr_scene
    g = torch.Generator().manual_seed(seed)
    V = gsr_scene.ring_camera(200, 120, 3).world_view_transform
    scales = torch.exp(torch.randn(P, 3, generator=g) * 0.7 - 3.0)
    rot = torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=1)
    means = torch.rand(P, 3, generator=g) * 3.0 - 1.5
    special = [(.1, .2, .3), (.2, .1, .3), (.3, .2, .1), (.1, .1, .3), (.3, .1, .1), (.2, .2, .2)]
    for i, s in enumerate(special[:P]):
        scales[i] = torch.tensor(s)
    if P > 7:
        rot[6] = 0
        rot[7] *= 3.7
    for _ in range(200):   # redraw the means of the Gaussians whose normal is nearly perpendicular to the viewing ray
        cos = tn.gaussian_normals(scales, rot, means, V, parts=True)[3]
        near = (cos.abs() < 0.05) & (rot.abs().sum(1) > 0)
        if not near.any():
            break
        means[near] = torch.rand(int(near.sum()), 3, generator=g) * 3.0 - 1.5
    return scales, rot, means, V


@pytest.mark.parametrize("space", ["view", "world"])
@pytest.mark.parametrize("P", [1, 63, 257])
def test_gaussian_normals_match_the_restatement(P, space):
    from fused_geometry import gaussian_normals
    scales, rot, means, V = _gaussian_case(P)
    ref, k, sign, cos = tn.gaussian_normals(scales, rot, means, V, space, parts=True)
    has_normal = rot.abs().sum(1) > 0
    assert float(cos[has_normal].abs().min()) >= 0.05      # every Gaussian: the zero quaternion has no normal, so no sign to decide
    if P > 7:
        assert set(k.tolist()) == {0, 1, 2} and k[:6].tolist() == [0, 1, 2, 0, 1, 0]
        assert (sign > 0).any() and (sign < 0).any()       # both branches of the flip
        assert not bool(has_normal[6]) and abs(float(rot[7].norm()) - 3.7) < 1e-5
    G = torch.randn(P, 3, generator=torch.Generator().manual_seed(P))
    q64 = rot.double().requires_grad_(True)
    out64 = tn.gaussian_normals(scales, q64, means, V, space)
    (out64 * G.double()).sum().backward()
    q32 = rot.clone().requires_grad_(True)
    out32 = tn.gaussian_normals(scales, q32, means, V, space, dtype=torch.float32)
    (out32 * G).sum().backward()
    to = lambda t: t.to(DEV)
    q = to(rot).requires_grad_(True)
    out = gaussian_normals(to(scales), q, to(means), to(V), space)
    assert out.shape == (P, 3) and out.dtype == torch.float32
    (out * to(G)).sum().backward()
    _check(f"gaussian normals P={P} {space}", out.detach(), out64.detach(), out32.detach(), grad=False)
    _check(f"gaussian normals P={P} {space} dL/drotations", q.grad, q64.grad, q32.grad, grad=True)
    assert float((q.grad * q.detach()).sum(1).abs().max()) <= 1e-5 * float(q.grad.abs().max())   # through the normalisation
    if P > 7:
        assert float(out[6].abs().max()) == 0 and float(q.grad[6].abs().max()) == 0               # the zero quaternion
    # the raw log-scales choose the same axes; no_grad works
    with torch.no_grad():
        assert torch.equal(gaussian_normals(to(torch.log(scales)), to(rot), to(means), to(V), space), out.detach())


def test_gaussian_normals_of_no_gaussian():
    from fused_geometry import gaussian_normals
    e = lambda *s: torch.zeros(*s, device=DEV)
    q = e(0, 4).requires_grad_(True)
    out = gaussian_normals(e(0, 3), q, e(0, 3), torch.eye(4, device=DEV))
    assert out.shape == (0, 3)
    out.sum().backward()
    assert q.grad.shape == (0, 4)


# ---- the stencil and the loss ----------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (5, 2), (3, 3), (70, 37), (200, 120)]   # (W, H): no interior pixel, one, two 64 x 16 tiles and a rest in each axis, the smoke size


def _depth(kind, W, H):
    """float32 (H, W) view-space depth"""
    tany = TANX * H / W
    if kind == "plane":
        return tn.plane_depth(W, H, TANX, tany)[0].float()
    X = ((2 * torch.arange(W, dtype=torch.float64) + 1) / W - 1)[None, :] * TANX
    Y = ((2 * torch.arange(H, dtype=torch.float64) + 1) / H - 1)[:, None] * tany
    if kind == "sphere":   # the cap of a sphere of radius 2.5 around (0, 0, 6); no depth (0) beside it
        rr, cr = X * X + Y * Y + 1, 6.0
        disc = cr * cr - rr * (36.0 - 6.25)
        return torch.where(disc > 0, (cr - disc.clamp_min(0).sqrt()) / rr, torch.zeros_like(rr)).float()
    g = torch.Generator().manual_seed(W * 1000 + H)
    z = torch.full((H, W), 4.0, dtype=torch.float64)
    for _ in range(4):   # smooth and random
        fx, fy, ph, am = (float(v) for v in torch.rand(4, generator=g))
        z = z + (0.2 + 0.4 * am) * torch.sin(6 * fx * X / TANX + 5 * fy * Y / max(tany, 1e-9) + 6.28 * ph)
    z = z.clamp(2.0, 6.0).float()
    z[H // 3:H // 2, W // 4:W // 2] = 0.0          # a rectangular hole
    if H > 4 and W > 4:
        z[(2 * H) // 3, (3 * W) // 4] = float("inf")
    return z


@pytest.mark.parametrize("kind", ["plane", "sphere", "random"])
@pytest.mark.parametrize("W,H", SIZES)
def test_depth_normals_and_loss_match_the_restatement(W, H, kind):
    from fused_geometry import depth_normals, normal_consistency_loss
    tany = TANX * H / W
    z = _depth(kind, W, H)
    g = torch.Generator().manual_seed(11)
    G = torch.randn(3, H, W, generator=g)
    N = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0) * (0.5 + torch.rand(1, H, W, generator=g))
    A = torch.rand(1, H, W, generator=g)
    up = 2.5   # a non-unit upstream factor
    to = lambda t: t.to(DEV)

    def reference(dtype):
        zr = z.clone().requires_grad_(True)
        nd = tn.depth_normals(zr, TANX, tany, dtype)
        (nd * G.to(dtype)).sum().backward()
        res = {"n": nd.detach(), "dz": zr.grad.clone()}
        for name, alpha in (("a", A), ("1", None)):
            zr, Nr = z.clone().requires_grad_(True), N.clone().requires_grad_(True)
            loss = tn.normal_consistency_loss(Nr, zr, alpha, TANX, tany, dtype)
            (up * loss).backward()
            res["loss" + name], res["dN" + name], res["dZ" + name] = loss.detach().reshape(1), Nr.grad, zr.grad
        return res
    r64, r32 = reference(torch.float64), reference(torch.float32)
    if kind == "plane" and W >= 3 and H >= 3:   # the analytic normal itself
        n_true = tn.plane_depth(W, H, TANX, tany)[1]
        assert float((r64["n"][:, 1:-1, 1:-1] - n_true[:, None, None]).abs().max()) < 1e-5

    zd = to(z).requires_grad_(True)
    nd = depth_normals(zd, TANX, tany)
    assert nd.shape == (3, H, W)
    (nd * to(G)).sum().backward()
    tag = f"{kind} {W}x{H}"
    _check(f"depth normals {tag}", nd.detach(), r64["n"], r32["n"], grad=False)
    _check(f"depth normals {tag} dL/ddepth", zd.grad, r64["dz"], r32["dz"], grad=True)
    assert torch.equal((nd.detach().cpu() == 0).all(0), (r64["n"] == 0).all(0))   # the same pixels have no normal: border, holes' neighbours
    assert torch.equal(depth_normals(to(z)[None], TANX, tany), nd.detach())   # (1, H, W)
    for name, alpha in (("a", A), ("1", None)):
        zd, Nd = to(z)[None].requires_grad_(True), to(N).requires_grad_(True)
        loss = normal_consistency_loss(Nd, zd, None if alpha is None else to(alpha), TANX, tany)
        assert loss.dim() == 0
        (up * loss).backward()
        assert zd.grad.shape == (1, H, W)
        _check(f"loss {tag} alpha={name}", loss.detach().reshape(1), r64["loss" + name], r32["loss" + name], grad=False)
        _check(f"loss {tag} alpha={name} dL/dnormal_map", Nd.grad, r64["dN" + name], r32["dN" + name], grad=True)
        _check(f"loss {tag} alpha={name} dL/ddepth", zd.grad[0], r64["dZ" + name], r32["dZ" + name], grad=True)


def test_loss_ignores_the_normal_map_where_there_is_no_depth_normal_and_runs_twice_with_the_same_bits():
    from fused_geometry import depth_normals, normal_consistency_loss
    W, H = 200, 120
    tany = TANX * H / W
    z = _depth("random", W, H).to(DEV)
    g = torch.Generator().manual_seed(12)
    N, A, G = (torch.randn(3, H, W, generator=g).to(DEV), torch.rand(H, W, generator=g).to(DEV), torch.randn(3, H, W, generator=g).to(DEV))

    def run(Nin):
        zd, Nd = z.clone().requires_grad_(True), Nin.clone().requires_grad_(True)
        loss = normal_consistency_loss(Nd, zd, A, TANX, tany)
        loss.backward()
        z2 = z.clone().requires_grad_(True)
        nd = depth_normals(z2, TANX, tany)
        (nd * G).sum().backward()
        return loss.detach(), Nd.grad, zd.grad, nd.detach(), z2.grad
    first, second = run(N), run(N)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    # whatever the normal map holds where there is no depth normal, it does not enter
    bad = N.clone()
    bad[:, (first[3] == 0).all(0)] = float("nan")
    third = run(bad)
    for a, b in zip(first, third):
        assert torch.equal(a, b)
    # only the loss's own inputs decide: without requires_grad nothing but the value is produced
    with torch.no_grad():
        assert torch.equal(normal_consistency_loss(N, z, A, TANX, tany), first[0])


# ---- render(normals=True) --------------------------------------------------------------------------------------------------------------
def _model(kw):
    import gsr_model
    import gsr_scene
    scene, cam = gsr_scene.make_scene(2000, -3.0, sh_degree=3, seed=3), gsr_scene.make_camera(200, 120)
    pc = gsr_model.GaussianParams.from_activated(scene.means3D, scene.shs, scene.scales, scene.rotations, scene.opacities, device=DEV,
                                                 max_sh_degree=3, active_sh_degree=3)
    camd = cam._replace(world_view_transform=cam.world_view_transform.to(DEV), full_proj_transform=cam.full_proj_transform.to(DEV),
                        camera_center=cam.camera_center.to(DEV))
    return scene, cam, camd, pc, gsr_model.pipeline_params(**kw), scene.bg.to(DEV)


def _own_normals(pc, kw, V, space="view"):
    from fused_geometry import gaussian_normals
    scales, rot = (pc._scaling, pc._rotation) if kw else (pc.get_scaling, pc.get_rotation)
    return gaussian_normals(scales, rot, pc.get_xyz, V, space)


@pytest.mark.parametrize("kw", [{}, dict(fused_activations=True)], ids=["activated", "leaf"])
def test_render_normals(kw):
    from fused_geometry import normal_consistency_loss
    from gaussian_renderer import render
    scene, cam, camd, pc, pipe, bg = _model(kw)
    P, H, W = 2000, cam.image_height, cam.image_width
    base = {"render", "viewspace_points", "visibility_filter", "radii", "depth", "alpha"}
    with torch.no_grad():
        plain = render(camd, pc, pipe, bg, depth_alpha="depth")
        r = render(camd, pc, pipe, bg, depth_alpha="depth", normals=True)
        assert set(r) == base | {"normal"} and r["normal"].shape == (3, H, W)
        own = render(camd, pc, pipe, bg, depth_alpha="depth", features=_own_normals(pc, kw, camd.world_view_transform))
        assert torch.equal(r["normal"], own["features"])
        assert float(r["normal"].abs().max()) > 0.1
        uf = torch.randn(P, 2, generator=torch.Generator().manual_seed(4)).to(DEV)
        with_uf = render(camd, pc, pipe, bg, depth_alpha="depth", features=uf)
        both = render(camd, pc, pipe, bg, depth_alpha="depth", features=uf, normals=True)
        assert set(both) == base | {"normal", "features"} and both["features"].shape == (2, H, W)
        assert torch.equal(both["features"], with_uf["features"]) and torch.equal(both["normal"], r["normal"])
        for res in (r, both):
            for key in ("render", "depth", "alpha", "radii"):
                assert torch.equal(res[key], plain[key]), key
        assert set(render(camd, pc, pipe, bg, depth_alpha="depth", normals=False)) == base
        assert set(render(camd, pc, pipe, bg, normals=True)) == (base - {"depth", "alpha"}) | {"normal"}
    # rotations.grad of a loss on colour plus the consistency loss against the explicit composition: the caller's own
    # gaussian_normals() as features= under the same loss.  rotations.grad is a two-term fp32 sum (the rasterizer's share and the
    # normals'), whose order autograd may choose differently
    dpix = torch.randn(3, H, W, generator=torch.Generator().manual_seed(5)).to(DEV)
    tanx, tany = cam.tanfovx, cam.tanfovy

    def grad_of(res, normal):
        for p in pc.parameters():
            p.grad = None
        surface = res["depth"] / res["alpha"].detach().clamp_min(1e-3)
        ((res["render"] * dpix).sum() + 0.7 * normal_consistency_loss(normal, surface, res["alpha"], tanx, tany)).backward()
        return pc._rotation.grad.clone()
    r = render(camd, pc, pipe, bg, depth_alpha="depth", normals=True)
    total = grad_of(r, r["normal"])
    e = render(camd, pc, pipe, bg, depth_alpha="depth", features=_own_normals(pc, kw, camd.world_view_transform))
    explicit = grad_of(e, e["features"])
    c = render(camd, pc, pipe, bg, depth_alpha="depth")
    for p in pc.parameters():
        p.grad = None
    (c["render"] * dpix).sum().backward()
    assert float((total - pc._rotation.grad).abs().max()) > 1e-3 * float(total.abs().max())   # the term reaches the rotations
    err, gmax = float((total - explicit).abs().max()), float(total.abs().max())
    print(f"render(normals=True) {kw}: rotations.grad err {err:.3e} of max {gmax:.3e}")
    assert err <= 1e-6 * gmax


@pytest.mark.parametrize("kw", [{}, dict(fused_activations=True)], ids=["activated", "leaf"])
def test_render_normals_with_camera_grads(kw):
    """With camera_grads the normals are rotated into view space in torch, so world_view_transform gets the rotation's gradient on top
    of the one through the blend weights.  The second is the feature pass's own (test_features_gpu.py, test_camera_grads_gpu.py) and is
    taken from a render with the kernel's view-space normals as detached features; the first is the float64 restatement's."""
    from gaussian_renderer import render
    scene, cam, camd, pc, pipe, bg = _model(kw)
    H, W = cam.image_height, cam.image_width
    G = torch.randn(3, H, W, generator=torch.Generator().manual_seed(6)).to(DEV)
    VA = camd.world_view_transform.clone().requires_grad_(True)
    rA = render(camd._replace(world_view_transform=VA), pc, pipe, bg, depth_alpha="depth", normals=True, camera_grads=True)
    (rA["normal"] * G).sum().backward()
    VB = camd.world_view_transform.clone().requires_grad_(True)
    nv = _own_normals(pc, kw, camd.world_view_transform).detach().requires_grad_(True)
    rB = render(camd._replace(world_view_transform=VB), pc, pipe, bg, depth_alpha="depth", features=nv, camera_grads=True)
    assert float((rA["normal"] - rB["features"]).abs().max()) <= 1e-5   # torch's rotation of the world-space normals against the kernel's
    (rB["features"] * G).sum().backward()
    scales = (pc._scaling if kw else pc.get_scaling).detach().cpu()
    rot, xyz, g_n = pc._rotation.detach().cpu(), pc.get_xyz.detach().cpu(), nv.grad.cpu()
    rotation = {}
    for dtype in (torch.float64, torch.float32):
        V = cam.world_view_transform.to(dtype).requires_grad_(True)
        (tn.gaussian_normals(scales, rot, xyz, V, "view", dtype) * g_n.to(dtype)).sum().backward()
        rotation[dtype] = V.grad
    assert float(rotation[torch.float64].abs().max()) > 0
    ref64 = VB.grad.double().cpu() + rotation[torch.float64]
    ref32 = VB.grad.cpu() + rotation[torch.float32]
    _check(f"render(normals=True, camera_grads=True) {kw} dL/dworld_view_transform", VA.grad, ref64, ref32, grad=True)
