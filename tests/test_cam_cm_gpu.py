"""GPU: camera gradients under a camera model (include/gsr_cam_cm.h, `camera_model_grads=`) -- dL/dviewmatrix, dL/dcampos and
dL/d(fx, fy, cx, cy) -- against the float64 autograd reference of tests/torch_splat_cam_cm.py, against the merged camera gradients of
the default path at the default intrinsics, their exact zeros and bookkeeping, the wave and fold edges, two reference-free identities
at sizes that cross the fold's width, bitwise reproducibility, and a pose-plus-focal refinement through render().

Bar per output tensor: max |got - sum_g t_g| <= max(1e-5 max_entries sum_g |t_g|, 3 d32), t_g the Gaussians' own terms
in float64 and d32 the distance of the helper's float32 run from its float64 run on the same discrete state.  Upstream gradients are
zero on the fragile pixels (margin 2e-5); radii are compared off the fragile-radius Gaussians.  At most 10 % of the pixels and 1 % of
the Gaussians may be excluded: asserted in every test that excludes anything.  Every error is printed beside its bar."""
import math

import pytest
import torch

import __graft_entry__  # noqa: F401
import torch_splat_cam_cm as tcc
import torch_splat_camera_model as tcm
import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VM_ZEROS = [3, 7, 11, 15]
_REF = {}
PINHOLE_37x21 = ("pinhole", 33.0, 31.0, 12.3, 13.9)   # an off-centre principal point on an image that is no multiple of the tile


def caps(st):
    assert float(st["fragile"].double().mean()) <= 0.10, "more than 10 % of the pixels are fragile"
    assert float(st["fragile_radius"].double().mean()) <= 0.01, "more than 1 % of the Gaussians have a fragile radius"


def _scene(name):
    if name == "base":
        return tcm.base_scene() + (tcm.PINHOLE_OFFCENTRE,)
    if name == "guard":
        return tcm.guard_scene()[:3]
    if name == "fisheye":
        return tcm.fisheye_scene()
    if name == "offcentre37x21":
        return tcm.base_scene(300, 37, 21) + (PINHOLE_37x21,)
    if name == "default":
        scene, cam = tcm.base_scene()
        return scene, cam, tcm.default_model(cam.image_width, cam.image_height, cam.tanfovx, cam.tanfovy)
    raise KeyError(name)


def _leaf_tensors(scene):
    """the optimiser's leaves of a scene: logits, log-scales, unnormalised quaternions, split SH"""
    op = scene.opacities.double().clamp(1e-4, 1 - 1e-4)
    g = torch.Generator().manual_seed(8)
    return dict(means3D=scene.means3D, means2D=torch.zeros_like(scene.means3D), features_dc=scene.shs[:, :1].contiguous(),
                features_rest=scene.shs[:, 1:].contiguous(), opacity=torch.log(op / (1 - op)).float(), scaling=torch.log(scene.scales),
                rotation=scene.rotations * (0.5 + torch.rand(scene.rotations.shape[0], 1, generator=g)))


VARIANTS = {   # inputs of the helper, keywords of both sides, what is in the loss, leaf mode
    "sh": ("sh", {}, ("image",), False),
    "colors_precomp": ("colors", {}, ("image",), False),
    "cov3D_precomp": ("cov", {}, ("image",), False),
    "antialiasing": ("sh", dict(antialiasing=True), ("image",), False),
    "depth": ("sh", dict(depth_mode="depth"), ("depth", "alpha"), False),
    "invdepth": ("sh", dict(depth_mode="invdepth"), ("depth", "alpha"), False),
    "leaf": ("sh", {}, ("image",), True),
    "leaf_aa_invdepth": ("sh", dict(antialiasing=True, depth_mode="invdepth"), ("image", "depth", "alpha"), True),
}


def reference(name, variant):
    """Scene, discrete state, upstream gradients and the float64 camera terms of a case, computed once and left unchanged."""
    key = (name, variant)
    if key in _REF:
        return _REF[key]
    scene, cam, cm = _scene(name)
    inputs, kw, in_loss, leaf = VARIANTS[variant]
    leaves = None
    if leaf:   # the camera sees the activated leaves
        leaves = _leaf_tensors(scene)
        scene = scene._replace(rotations=torch.nn.functional.normalize(leaves["rotation"], dim=1),
                               opacities=torch.sigmoid(leaves["opacity"]), scales=torch.exp(leaves["scaling"]))
    W, H = cam.image_width, cam.image_height
    inp = tcm.scene_inputs(scene, cam, inputs)
    st = tcc.probe_state(cm, W, H, scene.bg, 3, inp, **kw)
    caps(st)
    shapes = dict(image=(3, H, W), depth=(H, W), alpha=(H, W))
    dL = {k: tcm.fragile_free(st, shapes[k], seed) for seed, k in enumerate(in_loss, 1)}
    total, abs_total, d32, gg, _ = tcc.camera_terms(cm, W, H, scene.bg, 3, inp, dL, st, want_gaussians=True, **kw)
    _REF[key] = dict(scene=scene, cam=cam, cm=cm, inp=inp, kw=kw, st=st, dL=dL, total=total, abs_total=abs_total, d32=d32, gg=gg,
                     leaves=leaves)
    return _REF[key]


def _settings(scene, cam, W, H, debug=False, garbage=True):
    """projmatrix, tanfovx and tanfovy are ignored with a camera model -- hand over values nothing could render with"""
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    proj = torch.full((4, 4), float("nan")) if garbage else cam.full_proj_transform
    tx, ty = (123.0, -7.0) if garbage else (cam.tanfovx, cam.tanfovy)
    return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=tx, tanfovy=ty, bg=scene.bg.to(DEV), scale_modifier=1.0,
                                         viewmatrix=cam.world_view_transform.to(DEV), projmatrix=proj.to(DEV), sh_degree=3,
                                         campos=cam.camera_center.to(DEV), prefiltered=False, debug=debug)


NAMES = dict(shs="shs", colors_precomp="colors_precomp", scales="scales", rotations="rotations", cov3D_precomp="cov3D_precomp")


def hip(scene, cam, cm, dL, inp=None, mode="tensor", need=(True, True, True), leaves=None, antialiasing=False, depth_mode=None,
        debug=False):
    """One forward + backward on the GPU.  mode: "tensor" (camera_model_grads = the intrinsics tensor), "true" (= True), "false"
    (= False), "off" (no keyword at all: the plain camera-model path).  need: requires_grad of (viewmatrix, campos, intrinsics).
    -> (outputs on the CPU, [dL/dviewmatrix, dL/dcampos, dL/dintrinsics] or Nones, the Gaussian gradients)"""
    from diff_gaussian_rasterization import GaussianRasterizer
    W, H = cam.image_width, cam.image_height
    st = _settings(scene, cam, W, H, debug)
    V, C = st.viewmatrix.clone().requires_grad_(need[0]), st.campos.clone().requires_grad_(need[1])
    K = torch.tensor([float(v) for v in cm[1:]], device=DEV).requires_grad_(need[2])
    st = st._replace(viewmatrix=V, campos=C)
    kw = {} if mode == "off" else dict(camera_model_grads={"tensor": K, "true": True, "false": False}[mode])
    if leaves is not None:
        from fused_params import rasterize_leaf_gaussians
        leaf = {k: v.to(DEV).clone().requires_grad_(True) for k, v in leaves.items()}
        out = rasterize_leaf_gaussians(leaf["means3D"], leaf["means2D"], leaf["features_dc"], leaf["features_rest"], leaf["opacity"],
                                       leaf["scaling"], leaf["rotation"], st, camera_model=cm, antialiasing=antialiasing,
                                       depth_alpha=depth_mode, **kw)
    else:
        inp = inp if inp is not None else tcm.scene_inputs(scene, cam, "sh")
        leaf = {k: v.to(DEV).clone().requires_grad_(True) for k, v in inp.items() if k not in ("V", "campos")}
        call = dict(means3D=leaf["means3D"], means2D=leaf["means2D"], opacities=leaf["opacities"])
        call.update({NAMES[k]: v for k, v in leaf.items() if k in NAMES})
        out = GaussianRasterizer(st, camera_model=cm, antialiasing=antialiasing, depth_alpha=depth_mode, **kw)(**call)
    keys = ["image", None, "depth", "alpha"]
    loss = sum((out[i] * dL[k].to(DEV).reshape(out[i].shape)).sum() for i, k in enumerate(keys[:len(out)]) if k in dL)
    loss.backward()
    torch.cuda.synchronize()
    return tuple(o.detach().cpu() for o in out), [V.grad, C.grad, K.grad], {k: v.grad for k, v in leaf.items()}


def check(got, ref, what):
    worst = 0.0
    for g, k in zip(got, ("V", "campos", "K")):
        total, scale, d32 = ref["total"][k], float(ref["abs_total"][k].max()), ref["d32"][k]
        err = float((g.detach().cpu().double().reshape(total.shape) - total).abs().max())
        bar = max(1e-5 * scale, 3 * d32)
        print(f"{what} dL/d{k}: err {err:.3e} bar {bar:.3e} (scale {scale:.3e}, d32 {d32:.3e})")
        util.parity_log(f"cam_cm {what}: dL/d{k} {err:.3e} / {bar:.3e}")
        assert err <= bar, (what, k, err, bar)
        worst = max(worst, err / bar if bar > 0 else 0.0)
    assert all(float(got[0].reshape(-1)[i]) == 0.0 for i in VM_ZEROS)
    return worst


def same_gaussian_grads(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k


# ---- 1. float64 parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["base", "guard", "fisheye", "offcentre37x21"])
def test_against_float64_autograd(name, variant):
    ref = reference(name, variant)
    scene, cam, cm, st = ref["scene"], ref["cam"], ref["cm"], ref["st"]
    caps(st)
    run = dict(inp=ref["inp"], leaves=ref["leaves"], antialiasing=ref["kw"].get("antialiasing", False), depth_mode=ref["kw"].get("depth_mode"))
    out, got, gg = hip(scene, cam, cm, ref["dL"], **run)
    bad = (out[1].to(torch.int32) != st["radii"]) & ~st["fragile_radius"]
    assert not bool(bad.any()), bad.nonzero().flatten().tolist()[:8]
    assert got[0].shape == (4, 4) and got[1].shape == (3,) and got[2].shape == (4,)
    check(got, ref, f"{name} {variant}")
    if variant == "colors_precomp":
        assert torch.equal(got[1], torch.zeros_like(got[1]))
    elif "image" in ref["dL"]:   # (the maps alone do not reach the colours)
        assert float(got[1].abs().max()) > 0
    assert float(got[2].abs().min()) > 0
    # the Gaussian gradients are those of the plain camera-model path, bit for bit
    _, none, plain = hip(scene, cam, cm, ref["dL"], mode="off", **run)
    assert none == [None, None, None]
    same_gaussian_grads(gg, plain)


# ---- 2. against the merged camera gradients of the default path ----------------------------------------------------------------------------
def test_default_intrinsics_against_camera_grads_of_the_default_path():
    """A pinhole at the default intrinsics is the default camera; with PM = V Proj, the default path's dL/dV + dL/dPM Proj^T is the
    total derivative with respect to V, and campos enters the same way."""
    from diff_gaussian_rasterization import GaussianRasterizer
    ref = reference("default", "sh")
    scene, cam, cm, dL = ref["scene"], ref["cam"], ref["cm"], ref["dL"]
    caps(ref["st"])
    _, got, _ = hip(scene, cam, cm, dL)
    check(got, ref, "default intrinsics vs float64")
    st = util.hip_settings(scene, cam, 3, torch.device(DEV))
    cams = [t.clone().requires_grad_(True) for t in (st.viewmatrix, st.projmatrix, st.campos)]
    st = st._replace(viewmatrix=cams[0], projmatrix=cams[1], campos=cams[2])
    leaf = lambda t: t.to(DEV).clone().requires_grad_(True)
    means = leaf(scene.means3D)
    color, _ = GaussianRasterizer(st, camera_grads=True)(means3D=means, means2D=torch.zeros_like(means, requires_grad=True),
                                                         opacities=leaf(scene.opacities), shs=leaf(scene.shs), scales=leaf(scene.scales),
                                                         rotations=leaf(scene.rotations))
    (color * dL["image"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    dV, dPM, dC = (c.grad.cpu().double() for c in cams)
    proj = torch.linalg.solve(cam.world_view_transform.double(), cam.full_proj_transform.double())   # PM = V @ proj
    want = dV + dPM @ proj.t()
    for g, w, k in ((got[0], want, "V"), (got[1], dC, "campos")):
        err = float((g.cpu().double() - w).abs().max())
        bar = max(1e-5 * float(ref["abs_total"][k].max()), 3 * ref["d32"][k])
        print(f"default intrinsics vs camera_grads of the default path, dL/d{k}: err {err:.3e} bar {bar:.3e}")
        util.parity_log(f"cam_cm vs camera_grads: dL/d{k} {err:.3e} / {bar:.3e}")
        assert err <= bar, (k, err, bar)


# ---- 3. exactness and bookkeeping ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["guard", "fisheye"])
def test_bookkeeping(name):
    ref = reference(name, "sh")
    scene, cam, cm, dL = ref["scene"], ref["cam"], ref["cm"], ref["dL"]
    out, full, gg = hip(scene, cam, cm, dL)
    off_out, _, plain = hip(scene, cam, cm, dL, mode="off")
    # only the intrinsics tensor requires a gradient
    _, got, g1 = hip(scene, cam, cm, dL, need=(False, False, True))
    assert got[0] is None and got[1] is None and torch.equal(got[2], full[2])
    same_gaussian_grads(g1, plain)
    # only the view matrix; only campos
    _, got, _ = hip(scene, cam, cm, dL, need=(True, False, False))
    assert torch.equal(got[0], full[0]) and got[1] is None and got[2] is None
    _, got, _ = hip(scene, cam, cm, dL, need=(False, True, False))
    assert got[0] is None and torch.equal(got[1], full[1]) and got[2] is None
    # nothing requires a gradient: the plain camera-model kernels
    _, got, g0 = hip(scene, cam, cm, dL, need=(False, False, False))
    assert got == [None, None, None]
    same_gaussian_grads(g0, plain)
    # camera_model_grads=True: the same view and campos gradients, no handle for the intrinsics
    _, got, gt = hip(scene, cam, cm, dL, mode="true")
    assert torch.equal(got[0], full[0]) and torch.equal(got[1], full[1]) and got[2] is None
    same_gaussian_grads(gt, plain)
    # camera_model_grads=False is the call without the keyword, bit for bit
    f_out, got, gf = hip(scene, cam, cm, dL, mode="false")
    assert got == [None, None, None]
    assert all(torch.equal(a, b) for a, b in zip(f_out, off_out)) and all(torch.equal(a, b) for a, b in zip(out, off_out))
    same_gaussian_grads(gf, plain)


def test_debug_compares_the_tensor_with_the_model():
    from diff_gaussian_rasterization import CameraModel, GaussianRasterizer
    ref = reference("fisheye", "sh")
    scene, cam, cm = ref["scene"], ref["cam"], ref["cm"]
    K = torch.tensor([float(v) for v in cm[1:]], device=DEV, requires_grad=True)
    assert CameraModel.from_tensor(cm[0], K) == CameraModel(cm[0], *(float(v) for v in K.detach().cpu()))   # (float32 values)
    leaf = {k: v.to(DEV) for k, v in ref["inp"].items() if k not in ("V", "campos")}
    call = dict(means3D=leaf["means3D"], means2D=leaf["means2D"], opacities=leaf["opacities"], shs=leaf["shs"], scales=leaf["scales"],
                rotations=leaf["rotations"])
    st = _settings(scene, cam, cam.image_width, cam.image_height, debug=True)
    GaussianRasterizer(st, camera_model=cm, camera_model_grads=K)(**call)
    with pytest.raises(ValueError, match="camera_model_grads"):
        GaussianRasterizer(st, camera_model=cm, camera_model_grads=K.detach() * 1.01)(**call)


# ---- 4. launch edges -------------------------------------------------------------------------------------------------------------------------
def _identities(got, gg, cam, W, H):
    """The shift identity sum_g dL/dmean_g[k] = sum_i dL/dV[12+i] V[4k+i] - dL/dcampos[k] to 1e-5 sum_g |dL/dmean_g[k]|, and the
    principal-point identity dL/dcx = sum_g du_g, du_g = means2D.grad[g, 0] / (0.5 W), to 1e-5 sum_g |du_g| (cy likewise)."""
    V = cam.world_view_transform.double().reshape(-1)
    dV, dC, dK = (g.detach().cpu().double().reshape(-1) for g in got)
    dm, d2 = gg["means3D"].detach().cpu().double(), gg["means2D"].detach().cpu().double()
    for k in range(3):
        lhs = float(dm[:, k].sum())
        rhs = float(sum(dV[12 + i] * V[4 * k + i] for i in range(3)) - dC[k])
        bar = 1e-5 * float(dm[:, k].abs().sum())
        print(f"shift identity axis {k}: lhs {lhs:.6e} rhs {rhs:.6e} diff {abs(lhs - rhs):.3e} bar {bar:.3e}")
        assert abs(lhs - rhs) <= bar, (k, lhs, rhs, bar)
    for j, S in ((0, W), (1, H)):
        du = d2[:, j] / (0.5 * S)
        lhs, rhs, bar = float(dK[2 + j]), float(du.sum()), 1e-5 * float(du.abs().sum())
        print(f"principal-point identity axis {j}: lhs {lhs:.6e} rhs {rhs:.6e} diff {abs(lhs - rhs):.3e} bar {bar:.3e}")
        assert abs(lhs - rhs) <= bar, (j, lhs, rhs, bar)


MODELS = {"pinhole": tcm.PINHOLE_OFFCENTRE, "fisheye": tcm.FISHEYE}


@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
@pytest.mark.parametrize("P", [0, 1, 63, 64, 65])
def test_wave_edges(P, model):
    import gsr_scene
    scene, cam, cm = gsr_scene.make_scene(P, -1.0, sh_degree=3, seed=2), gsr_scene.make_camera(40, 24), MODELS[model]
    dL = {"image": torch.randn(3, 24, 40, generator=torch.Generator().manual_seed(1))}
    _, got, gg = hip(scene, cam, cm, dL)
    assert got[0].shape == (4, 4) and got[1].shape == (3,) and got[2].shape == (4,)
    assert all(bool(torch.isfinite(g).all()) for g in got)
    if P == 0:
        assert all(torch.equal(g, torch.zeros_like(g)) for g in got)
        return
    _identities(got, gg, cam, 40, 24)
    _, _, plain = hip(scene, cam, cm, dL, mode="off")
    same_gaussian_grads(gg, plain)


@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
def test_all_culled_scene_gives_exact_zeros(model):
    import gsr_scene
    scene, cam = gsr_scene.make_scene(130, -1.0, sh_degree=3, seed=2), gsr_scene.make_camera(40, 24)
    scene = scene._replace(means3D=scene.means3D - torch.tensor([0.0, 0.0, 20.0]))   # all behind the camera
    _, got, _ = hip(scene, cam, MODELS[model], {"image": torch.ones(3, 24, 40)})
    assert all(torch.equal(g, torch.zeros_like(g)) for g in got)


@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
def test_only_the_last_lane_of_the_last_wave_is_visible(model):
    import gsr_scene
    scene, cam = gsr_scene.make_scene(128, -1.0, sh_degree=3, seed=4), gsr_scene.make_camera(40, 24)
    means = scene.means3D - torch.tensor([0.0, 0.0, 20.0])
    means[127] = torch.tensor([0.1, -0.05, 0.2])
    scene = scene._replace(means3D=means)
    dL = {"image": torch.randn(3, 24, 40, generator=torch.Generator().manual_seed(1))}
    out, got, gg = hip(scene, cam, MODELS[model], dL)
    assert int((out[1] > 0).sum()) == 1 and int(out[1][127]) > 0
    assert all(float(g.abs().max()) > 0 for g in got)
    _identities(got, gg, cam, 40, 24)


@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
def test_cooperative_slot_runs_at_128x96(model):
    """48 tiles: splats of more than GSR_SLOT_COOP = 30 tiles take the wave-cooperative slot sum"""
    import gsr_scene
    scene, cam = gsr_scene.make_scene(2000, -2.5, sh_degree=3, seed=9), gsr_scene.make_camera(128, 96)
    scales = scene.scales.clone()
    scales[:3] = 2.0
    scene = scene._replace(scales=scales)
    cm = (model, 60.0, 58.0, 60.7, 50.2) if model == "pinhole" else (model, 45.0, 45.0, 64.3, 47.6)
    inp = tcm.scene_inputs(scene, cam, "sh")
    st = tcc.probe_state(cm, 128, 96, scene.bg, 3, {k: v[:8] if k not in ("V", "campos") else v for k, v in inp.items()})
    minx, miny, maxx, maxy = st["rect"]
    assert int(((maxx - minx) * (maxy - miny))[:3].max()) > 30, "no splat of more than GSR_SLOT_COOP tiles"
    dL = {"image": torch.randn(3, 96, 128, generator=torch.Generator().manual_seed(2))}
    _, got, gg = hip(scene, cam, cm, dL)
    _identities(got, gg, cam, 128, 96)
    _, _, plain = hip(scene, cam, cm, dL, mode="off")
    same_gaussian_grads(gg, plain)


# ---- 5. fold edges -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
@pytest.mark.parametrize("P", [20_011, 100_003])
def test_fold_at_size_and_reproducibility(P, model):
    """100 003 Gaussians are 1 563 rows, more than the fold's 1 024 threads.  Reference-free: the two identities, then a second run
    with the same bits, also behind the forwards that do not trim the lists or split the heavy tiles."""
    import gsr_scene
    from diff_gaussian_rasterization import _C
    scene, cam, cm = gsr_scene.make_scene(P, -2.5, sh_degree=3, seed=9), gsr_scene.make_camera(40, 24), MODELS[model]
    dL = {"image": torch.randn(3, 24, 40, generator=torch.Generator().manual_seed(2))}
    _, got, gg = hip(scene, cam, cm, dL)
    _identities(got, gg, cam, 40, 24)
    _, again, _ = hip(scene, cam, cm, dL)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    for flag in ("DEBUG_NO_TRIM", "DEBUG_NO_SPLIT"):
        runs = [hip(scene, cam, cm, dL, mode="true", debug=getattr(_C, flag))[1][:2] for _ in range(2)]
        assert all(torch.equal(a, b) for a, b in zip(*runs)) and float(runs[0][0].abs().max()) > 0
    _, _, plain = hip(scene, cam, cm, dL, mode="off")
    same_gaussian_grads(gg, plain)


# ---- 6. use ------------------------------------------------------------------------------------------------------------------------------------
def _pose_camera(cam, xi, dev):
    """The camera of `cam` moved by the 6-vector xi = (rotation vector, translation) in view space, in torch: world_view_transform
    and camera_center are functions of xi."""
    V0 = cam.world_view_transform.to(dev)            # (4,4), row-vector convention: p_view = (p, 1) @ V
    w, tr = xi[:3], xi[3:]
    zero = torch.zeros((), device=dev)
    K = torch.stack([torch.stack([zero, -w[2], w[1]]), torch.stack([w[2], zero, -w[0]]), torch.stack([-w[1], w[0], zero])])
    Rm = torch.linalg.matrix_exp(K)
    D = torch.cat([torch.cat([Rm.t(), torch.zeros(3, 1, device=dev)], 1), torch.cat([tr, torch.ones(1, device=dev)])[None]], 0)
    V = V0 @ D
    return cam._replace(world_view_transform=V, full_proj_transform=cam.full_proj_transform.to(dev), camera_center=torch.linalg.inv(V)[3, :3])


@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
def test_pose_and_focal_refinement_end_to_end(model):
    """render(..., camera_model=, camera_model_grads=intrinsics) with a camera built in torch from a 6-vector and the intrinsics from
    one focal scalar: 30 Adam steps on both, started a little off the pose and the focal length that produced the target, lower the
    L1 loss, the pose error and the focal error.

    The start.  A focal error ds is compensated to first order by a translation along the view axis of ds z (z about 4 here), so
    while it lasts it drags t_z away from the truth; the start keeps that drag below the pose error: ds = 0.003 (0.012 of drag at
    most) against |xi| = 0.0089, both parameters at Adam's lr 3e-4 (at most 0.009 of travel each in 30 steps).  The float64 helper
    of tests/torch_splat_cam_cm.py, stepped the same way on the CPU, goes |xi| 8.9e-3 -> 6.8e-3 (pinhole) and 6.0e-3 (fisheye) and
    ds 3.0e-3 -> 1.4e-3 and 1.3e-3 from this start; from ds = 0.01 at lr 5e-4 the same helper ends at |xi| 9.1e-3 / 8.9e-3, above
    where it began, with the loss a ninth of its start -- the ambiguity, not the gradients."""
    import gsr_model
    import gsr_scene
    from diff_gaussian_rasterization import CameraModel
    from gaussian_renderer import render
    dev = torch.device(DEV)
    scene = gsr_scene.make_scene(3000, -2.5, sh_degree=3, seed=21)
    cam = gsr_scene.make_camera(40, 24)
    cm0 = MODELS[model]
    pc = gsr_model.GaussianParams.from_activated(scene.means3D, scene.shs, scene.scales, scene.rotations, scene.opacities,
                                                 device=dev, active_sh_degree=3)
    pipe, bg = gsr_model.pipeline_params(), scene.bg.to(dev)
    with torch.no_grad():
        target = render(_pose_camera(cam, torch.zeros(6, device=dev), dev), pc, pipe, bg, camera_model=cm0)["render"]
    xi = torch.tensor([0.004, -0.003, 0.002, 0.005, -0.004, 0.003], device=dev, requires_grad=True)
    s = torch.tensor(1.003, device=dev, requires_grad=True)   # the focal scalar: fx = s fx0, fy = s fy0
    base = torch.tensor([float(v) for v in cm0[1:]], device=dev)
    opt = torch.optim.Adam([{"params": [xi], "lr": 3e-4}, {"params": [s], "lr": 3e-4}])
    losses, err0, f0 = [], float(xi.detach().norm()), abs(float(s.detach()) - 1.0)
    for _ in range(30):
        opt.zero_grad()
        intr = torch.cat([base[:2] * s, base[2:]])
        cm = CameraModel.from_tensor(model, intr)   # the one read-back of the step
        loss = (render(_pose_camera(cam, xi, dev), pc, pipe, bg, camera_model=cm, camera_model_grads=intr)["render"] - target).abs().mean()
        loss.backward()
        assert xi.grad is not None and bool(torch.isfinite(xi.grad).all()) and float(xi.grad.abs().max()) > 0
        assert s.grad is not None and bool(torch.isfinite(s.grad)) and float(s.grad.abs()) > 0
        opt.step()
        losses.append(float(loss.detach()))
    print(f"{model} pose + focal refinement: L1 {losses[0]:.4e} -> {losses[-1]:.4e}, |xi| {err0:.4e} -> {float(xi.detach().norm()):.4e}, "
          f"|s - 1| {f0:.4e} -> {abs(float(s.detach()) - 1.0):.4e}")
    assert losses[-1] < losses[0]
    assert float(xi.detach().norm()) < err0
    assert abs(float(s.detach()) - 1.0) < f0
