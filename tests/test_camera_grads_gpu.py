"""GPU: the camera gradients (include/gsr_cam.h, GaussianRasterizer(camera_grads=True)) against the float64 autograd reference of
tests/torch_splat_cam.py, their exact zeros, the wave and fold edges, a reference-free identity at sizes that cross the fold's
width, and bitwise reproducibility.

Bar per output tensor (the rule of tests/test_loss.py and DESIGN 6b): max |got - sum_g t_g| <= max(1e-5 max_entries sum_g |t_g|,
3 d32), t_g the Gaussians' own terms in float64 and d32 the distance of the helper's float32 run from its float64 run."""
import pytest
import torch

import __graft_entry__  # noqa: F401
import torch_splat_cam
import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VM_ZEROS = [3, 7, 11, 15]
PM_ZEROS = [2, 6, 10, 14]
_cache = {}


def _reference(variant):
    """Scene, oracle state, upstream gradients and the float64 terms of a variant, computed once."""
    if variant in _cache:
        return _cache[variant]
    scene, cam = torch_splat_cam.camera_test_scene()
    P = scene.means3D.shape[0]
    g = torch.Generator().manual_seed(11)
    colors = torch.rand(P, 3, generator=g) if variant == "colors_precomp" else None
    cov = None
    if variant == "cov3D_precomp":   # Sigma = R S^2 R^T in float64, rounded once
        r, x, y, z = scene.rotations.double().unbind(1)
        Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z),
                          1 - 2 * (x * x + z * z), 2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x),
                          1 - 2 * (x * x + y * y)], 1).reshape(P, 3, 3)
        M = Rm @ torch.diag_embed(scene.scales.double())
        S = M @ M.transpose(1, 2)
        cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).float()
    o = util.oracle_forward(scene, cam, 3, colors_precomp=colors, cov3D_precomp=cov, use_sh=colors is None, use_scale_rot=cov is None)
    dpix = util.fragile_free_dpix(o, cam, seed=3)
    assert float((dpix == 0).all(0).float().mean()) < 0.05, "the scene zeroes too many fragile pixels"
    assert int((o["radii"] == 0).sum()) >= 10, "the scene lost its culled Gaussians"
    inputs = dict(means3D=scene.means3D, opacities=scene.opacities, V=cam.world_view_transform, PM=cam.full_proj_transform,
                  campos=cam.camera_center)
    kw = {}
    if colors is None:
        inputs["shs"] = scene.shs
    else:
        kw["colors_precomp"] = colors
    if cov is None:
        inputs["scales"], inputs["rotations"] = scene.scales, scene.rotations
    else:
        kw["cov3D_precomp"] = cov
    dL = dpix
    if variant in ("antialiasing", "aa_invdepth"):
        kw["antialiasing"] = True
    if variant == "aa_invdepth":   # image and both maps in the loss
        kw["depth_mode"] = "invdepth"
        dL = (dpix, torch.randn(cam.image_height, cam.image_width, generator=g) * (dpix[0] != 0),
              torch.randn(cam.image_height, cam.image_width, generator=g) * (dpix[0] != 0))
    if variant == "invdepth":
        kw["depth_mode"] = "invdepth"
        dL = (torch.zeros_like(dpix), torch.randn(cam.image_height, cam.image_width, generator=g) * (dpix[0] != 0),
              torch.randn(cam.image_height, cam.image_width, generator=g) * (dpix[0] != 0))
    total, abs_total, d32 = torch_splat_cam.camera_terms(o, inputs, dL, **kw)
    assert torch_splat_cam.render.clamp_active >= 5, "the scene lost its clamped Gaussians"
    assert torch_splat_cam.render.max_tiles == 6, "no splat covers every tile"
    assert torch_splat_cam.render.subpixel >= 1, "the scene lost its sub-pixel Gaussian"
    _cache[variant] = (scene, cam, colors, cov, dL, total, abs_total, d32)
    return _cache[variant]


def _run(scene, cam, dL, camera_grads, colors=None, cov=None, antialiasing=False, depth_alpha=None, need=(True, True, True), D=3):
    """One forward + backward on the GPU -> (camera gradients or Nones, the Gaussian gradients)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device(DEV)
    leaf = lambda t: t.to(dev).clone().requires_grad_(True)
    inp = dict(means3D=leaf(scene.means3D), opacities=leaf(scene.opacities))
    inp["means2D"] = torch.zeros_like(inp["means3D"], requires_grad=True)
    if colors is None:
        inp["shs"] = leaf(scene.shs)
    else:
        inp["colors_precomp"] = leaf(colors)
    if cov is None:
        inp["scales"], inp["rotations"] = leaf(scene.scales), leaf(scene.rotations)
    else:
        inp["cov3D_precomp"] = leaf(cov)
    st = util.hip_settings(scene, cam, D, dev)
    cams = [t.clone().requires_grad_(n) for t, n in zip((st.viewmatrix, st.projmatrix, st.campos), need)]
    st = st._replace(viewmatrix=cams[0], projmatrix=cams[1], campos=cams[2])
    kw = dict(camera_grads=True) if camera_grads else {}
    out = GaussianRasterizer(st, antialiasing=antialiasing, depth_alpha=depth_alpha, **kw)(**inp)
    dL = dL if isinstance(dL, (tuple, list)) else (dL,)
    outs = (out[0],) + tuple(out[2:])
    loss = sum((o_ * d.to(dev).reshape(o_.shape)).sum() for o_, d in zip(outs, dL))
    loss.backward()
    torch.cuda.synchronize()
    return [c.grad for c in cams], {k: v.grad for k, v in inp.items()}


def _check_against_reference(got, total, abs_total, d32, label):
    for g, k in zip(got, ("V", "PM", "campos")):
        err = float((g.detach().cpu().double().reshape(total[k].shape) - total[k]).abs().max())
        bar = max(1e-5 * float(abs_total[k].max()), 3 * d32[k])
        print(f"{label} dL/d{k}: err {err:.3e} bar {bar:.3e} (scale {float(abs_total[k].max()):.3e}, d32 {d32[k]:.3e})")
        assert err <= bar, (label, k, err, bar)
    vm, pm = got[0].reshape(-1), got[1].reshape(-1)
    assert all(float(vm[i]) == 0.0 for i in VM_ZEROS) and all(float(pm[i]) == 0.0 for i in PM_ZEROS)


def _same_gaussian_grads(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("variant", ["default", "colors_precomp", "cov3D_precomp", "antialiasing", "invdepth"])
def test_against_float64_autograd(variant):
    scene, cam, colors, cov, dL, total, abs_total, d32 = _reference(variant)
    kw = dict(colors=colors, cov=cov, antialiasing=variant == "antialiasing", depth_alpha="invdepth" if variant == "invdepth" else None)
    got, gg = _run(scene, cam, dL, True, **kw)
    _check_against_reference(got, total, abs_total, d32, variant)
    if variant == "colors_precomp":
        assert torch.equal(got[2], torch.zeros_like(got[2]))
    _, plain = _run(scene, cam, dL, False, **kw)
    _same_gaussian_grads(gg, plain)


def test_only_viewmatrix_requires_grad():
    scene, cam, _, _, dL, total, abs_total, d32 = _reference("default")
    got, gg = _run(scene, cam, dL, True, need=(True, False, False))
    assert got[1] is None and got[2] is None
    err = float((got[0].cpu().double() - total["V"]).abs().max())
    assert err <= max(1e-5 * float(abs_total["V"].max()), 3 * d32["V"])
    _, plain = _run(scene, cam, dL, False)
    _same_gaussian_grads(gg, plain)


def test_none_requires_grad_runs_the_default_path():
    scene, cam, _, _, dL, *_ = _reference("default")
    got, gg = _run(scene, cam, dL, True, need=(False, False, False))
    assert got == [None, None, None]
    _, plain = _run(scene, cam, dL, False)
    _same_gaussian_grads(gg, plain)


@pytest.mark.parametrize("variant", ["default", "aa_invdepth"])
def test_leaf_mode_matches_the_reference(variant):
    """Leaf mode alone, and leaf + anti-aliasing + inverse depth together (image, D and A all in the loss): the leaves are the inverse
    activations of the scene's tensors, so the camera sees the same function as the reference."""
    from fused_params import rasterize_leaf_gaussians
    scene, cam, _, _, dL, total, abs_total, d32 = _reference(variant)
    kw = dict(depth_alpha="invdepth", antialiasing=True) if variant == "aa_invdepth" else {}
    dLs = dL if isinstance(dL, tuple) else (dL,)
    dev = torch.device(DEV)
    leaf = lambda t: t.to(dev).clone().requires_grad_(True)
    st = util.hip_settings(scene, cam, 3, dev)
    res = []
    for camera in (True, False):
        cams = [t.clone().requires_grad_(True) for t in (st.viewmatrix, st.projmatrix, st.campos)]
        s2 = st._replace(viewmatrix=cams[0], projmatrix=cams[1], campos=cams[2])
        op = scene.opacities.double()
        args = [leaf(scene.means3D), torch.zeros(scene.means3D.shape, device=dev, requires_grad=True), leaf(scene.shs[:, :1]),
                leaf(scene.shs[:, 1:]), leaf(torch.log(op / (1 - op)).float()), leaf(torch.log(scene.scales)), leaf(scene.rotations)]
        out = rasterize_leaf_gaussians(*args, s2, camera_grads=camera, **kw)
        sum((o_ * d.to(dev).reshape(o_.shape)).sum() for o_, d in zip((out[0],) + tuple(out[2:]), dLs)).backward()
        torch.cuda.synchronize()
        res.append(([c.grad for c in cams], [a.grad for a in args]))
    _check_against_reference(res[0][0], total, abs_total, d32, "leaf " + variant)
    assert res[1][0] == [None, None, None]
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65])
def test_wave_edges(P):
    import gsr_scene
    scene, cam = gsr_scene.make_scene(P, -1.0, sh_degree=3, seed=2), gsr_scene.make_camera(40, 24)
    dpix = torch.randn(3, 24, 40, generator=torch.Generator().manual_seed(1))
    got, gg = _run(scene, cam, dpix, True)
    assert got[0].shape == (4, 4) and got[1].shape == (4, 4) and got[2].shape == (3,)
    assert all(bool(torch.isfinite(g).all()) for g in got)
    if P == 0:
        assert all(torch.equal(g, torch.zeros_like(g)) for g in got)
        return
    # the shift identity of test_reduction_at_size, at the float32 scale of the sums
    _shift_identity(got, gg["means3D"], cam)
    _, plain = _run(scene, cam, dpix, False)
    _same_gaussian_grads(gg, plain)


def test_all_culled_scene_gives_exact_zeros():
    import gsr_scene
    scene, cam = gsr_scene.make_scene(130, -1.0, sh_degree=3, seed=2), gsr_scene.make_camera(40, 24)
    scene = scene._replace(means3D=scene.means3D - torch.tensor([0.0, 0.0, 20.0]))   # all behind the camera
    got, _ = _run(scene, cam, torch.ones(3, 24, 40), True)
    assert all(torch.equal(g, torch.zeros_like(g)) for g in got)


def test_only_the_last_lane_of_the_last_wave_is_visible():
    import gsr_scene
    scene, cam = gsr_scene.make_scene(128, -1.0, sh_degree=3, seed=4), gsr_scene.make_camera(40, 24)
    means = scene.means3D - torch.tensor([0.0, 0.0, 20.0])
    means[127] = torch.tensor([0.1, -0.05, 0.2])
    scene = scene._replace(means3D=means)
    dpix = torch.randn(3, 24, 40, generator=torch.Generator().manual_seed(1))
    got, gg = _run(scene, cam, dpix, True)
    assert float(got[0].abs().max()) > 0 and float(got[1].abs().max()) > 0 and float(got[2].abs().max()) > 0
    _shift_identity(got, gg["means3D"], cam)


def _shift_identity(got, dmeans, cam):
    """Translating the world by delta is the same function as shifting the camera.  With mean -> mean + delta: t = V^T (mean, 1)
    changes as if V[12 + i] grew by sum_k V[4 k + i] delta_k (i < 3; the rotation part of V, hence W, is untouched), p_hom as if
    PM[12 + r] grew by sum_k PM[4 k + r] delta_k (r = 0, 1, 3 reach the gradient), and the view direction mean - campos as if campos
    shrank by delta.  Differentiating at delta = 0:
      sum_g dL/dmean_g[k] = sum_{i<3} dL/dV[12+i] V[4k+i] + sum_{r in {0,1,3}} dL/dPM[12+r] PM[4k+r] - dL/dcampos[k]."""
    V, PM = cam.world_view_transform.double().reshape(-1), cam.full_proj_transform.double().reshape(-1)
    dV, dPM, dc = (g.detach().cpu().double().reshape(-1) for g in got)
    dm = dmeans.detach().cpu().double()
    for k in range(3):
        lhs = float(dm[:, k].sum())
        rhs = float(sum(dV[12 + i] * V[4 * k + i] for i in range(3)) + sum(dPM[12 + r] * PM[4 * k + r] for r in (0, 1, 3)) - dc[k])
        bar = 1e-5 * float(dm[:, k].abs().sum())
        print(f"shift identity axis {k}: lhs {lhs:.6e} rhs {rhs:.6e} diff {abs(lhs - rhs):.3e} bar {bar:.3e}")
        assert abs(lhs - rhs) <= bar, (k, lhs, rhs, bar)


def test_shift_identity_holds_on_the_float64_helper():
    """The identity of _shift_identity on the reference itself: if it failed here it would be wrong as written."""
    scene, cam, _, _, dL, total, *_ = _reference("default")
    o = util.oracle_forward(scene, cam, 3)
    m = scene.means3D.double().requires_grad_(True)
    img = torch_splat_cam.render(o, m, scene.scales, scene.rotations, scene.opacities, scene.shs, cam.world_view_transform,
                                 cam.full_proj_transform, cam.camera_center)
    (img * dL.double()).sum().backward()
    _shift_identity([total["V"], total["PM"], total["campos"]], m.grad, cam)


@pytest.mark.parametrize("P", [20_011, 100_003])
def test_reduction_at_size_and_reproducibility(P):
    """128 x 96 (48 tiles: splats of more than GSR_SLOT_COOP = 30 tiles take the cooperative run); 100 003 Gaussians are 1 563 rows,
    more than the fold's 1 024 threads.  Reference-free: the shift identity, then a second run with the same bits, also under the
    forwards that do not trim the lists or split the heavy tiles."""
    import gsr_scene
    scene, cam = gsr_scene.make_scene(P, -2.5, sh_degree=3, seed=9), gsr_scene.make_camera(128, 96)
    scales = scene.scales.clone()
    scales[:3] = 2.0
    scene = scene._replace(scales=scales)
    # a Gaussian's tile rectangle depends on itself alone: the oracle over the first eight shows the cooperative run is taken
    head = scene._replace(**{k: getattr(scene, k)[:8] for k in ("means3D", "scales", "rotations", "opacities", "shs")})
    assert int(util.oracle_forward(head, cam, 3)["tiles_touched"][:3].max()) > 30, "no splat of more than GSR_SLOT_COOP tiles"
    dpix = torch.randn(3, 96, 128, generator=torch.Generator().manual_seed(2))
    got, gg = _run(scene, cam, dpix, True)
    _shift_identity(got, gg["means3D"], cam)
    again, _ = _run(scene, cam, dpix, True)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    _, plain = _run(scene, cam, dpix, False)
    _same_gaussian_grads(gg, plain)


@pytest.mark.parametrize("flag", ["DEBUG_NO_TRIM", "DEBUG_NO_SPLIT"])
def test_reproducible_under_debug_forwards(flag):
    """Two runs give the same bits under the forwards that keep the reference's untrimmed lists / do not split heavy tiles."""
    import gsr_scene
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    dev = torch.device(DEV)
    scene, cam = gsr_scene.make_scene(20_011, -2.5, sh_degree=3, seed=9), gsr_scene.make_camera(128, 96)
    dpix = torch.randn(3, 96, 128, generator=torch.Generator().manual_seed(2)).to(dev)
    runs = []
    for _ in range(2):
        st = util.hip_settings(scene, cam, 3, dev, debug=getattr(_C, flag))
        cams = [t.clone().requires_grad_(True) for t in (st.viewmatrix, st.projmatrix, st.campos)]
        st = st._replace(viewmatrix=cams[0], projmatrix=cams[1], campos=cams[2])
        means = scene.means3D.to(dev).requires_grad_(True)
        color, _ = GaussianRasterizer(st, camera_grads=True)(
            means3D=means, means2D=torch.zeros_like(means, requires_grad=True), opacities=scene.opacities.to(dev),
            shs=scene.shs.to(dev), scales=scene.scales.to(dev), rotations=scene.rotations.to(dev))
        (color * dpix).sum().backward()
        torch.cuda.synchronize()
        runs.append([c.grad.clone() for c in cams])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert float(runs[0][0].abs().max()) > 0


def _pose_camera(cam, xi, dev):
    """The camera of `cam` moved by the 6-vector xi = (rotation vector, translation) in view space, in torch: world_view_transform,
    full_proj_transform and camera_center are functions of xi."""
    V0 = cam.world_view_transform.to(dev)            # (4,4), row-vector convention: p_view = (p, 1) @ V
    proj = torch.linalg.solve(V0.double(), cam.full_proj_transform.to(dev).double()).float()   # full = V @ proj
    w, tr = xi[:3], xi[3:]
    zero = torch.zeros((), device=dev)
    K = torch.stack([torch.stack([zero, -w[2], w[1]]), torch.stack([w[2], zero, -w[0]]), torch.stack([-w[1], w[0], zero])])
    Rm = torch.linalg.matrix_exp(K)
    D = torch.cat([torch.cat([Rm.t(), torch.zeros(3, 1, device=dev)], 1), torch.cat([tr, torch.ones(1, device=dev)])[None]], 0)
    V = V0 @ D
    return cam._replace(world_view_transform=V, full_proj_transform=V @ proj, camera_center=torch.linalg.inv(V)[3, :3])


def test_pose_refinement_end_to_end():
    """render(..., camera_grads=True) with a camera built in torch from a 6-vector: 30 Adam steps on the pose alone, started a few
    millimetres and a fraction of a degree off the pose that produced the target, lower the L1 loss and the pose error."""
    import gsr_model
    import gsr_scene
    from gaussian_renderer import render
    dev = torch.device(DEV)
    scene = gsr_scene.make_scene(3000, -2.5, sh_degree=3, seed=21)
    cam = gsr_scene.make_camera(128, 96)
    pc = gsr_model.GaussianParams.from_activated(scene.means3D, scene.shs, scene.scales, scene.rotations, scene.opacities,
                                                 device=dev, active_sh_degree=3)
    pipe, bg = gsr_model.pipeline_params(), scene.bg.to(dev)
    with torch.no_grad():
        target = render(_pose_camera(cam, torch.zeros(6, device=dev), dev), pc, pipe, bg)["render"]
    xi = torch.tensor([0.004, -0.003, 0.002, 0.005, -0.004, 0.003], device=dev, requires_grad=True)
    opt = torch.optim.Adam([xi], lr=3e-4)
    losses, err0 = [], float(xi.detach().norm())
    for _ in range(30):
        opt.zero_grad()
        loss = (render(_pose_camera(cam, xi, dev), pc, pipe, bg, camera_grads=True)["render"] - target).abs().mean()
        loss.backward()
        assert xi.grad is not None and bool(torch.isfinite(xi.grad).all()) and float(xi.grad.abs().max()) > 0
        opt.step()
        losses.append(float(loss))
    print(f"pose refinement: L1 {losses[0]:.4e} -> {losses[-1]:.4e}, |xi| {err0:.4e} -> {float(xi.detach().norm()):.4e}")
    assert losses[-1] < losses[0]
    assert float(xi.detach().norm()) < err0
