"""GPU: the camera models (include/gsr_camera_model.h) -- a pinhole with intrinsics and an equidistant fisheye -- against the default
path, against the float64 autograd helper tests/torch_splat_camera_model.py, and, by composition, against the CPU oracle.

Bars.  Image: 1e-5 on the pixels the helper (or the oracle) does not flag fragile.  Gradients, with upstream gradients zeroed on the
fragile pixels: max(1e-5 max|g|, 3 d32) per tensor, g the float64 gradient and d32 the distance of the helper's own float32 run from
it (the rule of tests/test_camera_grads_gpu.py).  In the float64 parity of the two models alone (test 4, check_grads(chain=True)),
scales and rotations, the end of the covariance chain, get no less than the band of tests/test_antialias_gpu.py,
max(5e-5, 10 x one split-pass sample) of the largest element, the sample being the float32 helper's own (tcm.split_sample): pinhole sh
rotations measured 1.25e-4 against 1.17e-4 by the plain rule.  Every other test keeps the plain rule for every tensor.  At most 10 % of the pixels and 1 % of the Gaussians may be excluded; both caps are
asserted here and, from the helper alone, in tests/test_camera_model_cpu.py.  Every error is printed beside its bar."""
import math

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
import torch_splat_camera_model as tcm
import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REF = {}   # references, computed once and shared


def _settings(scene, cam, W, H, garbage=False, debug=False):
    """garbage: projmatrix, tanfovx and tanfovy are ignored with a camera model -- hand over values nothing could render with"""
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    proj = torch.full((4, 4), float("nan")) if garbage else cam.full_proj_transform
    tx, ty = (123.0, -7.0) if garbage else (cam.tanfovx, cam.tanfovy)
    return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=tx, tanfovy=ty, bg=scene.bg.to(DEV), scale_modifier=1.0,
                                         viewmatrix=cam.world_view_transform.to(DEV), projmatrix=proj.to(DEV), sh_degree=3,
                                         campos=cam.camera_center.to(DEV), prefiltered=False, debug=debug)


NAMES = dict(shs="shs", colors_precomp="colors_precomp", scales="scales", rotations="rotations", cov3D_precomp="cov3D_precomp")


def hip(scene, cam, cm, dL=None, variant="sh", W=None, H=None, debug=False, stats=False, no_model=False, inputs=None, **kw):
    """GaussianRasterizer forward (+ backward for the loss sum(outputs * dL)) -> (outputs on the CPU, gradients dict in float64)"""
    from diff_gaussian_rasterization import GaussianRasterizer
    W, H = W or cam.image_width, H or cam.image_height
    inp = inputs if inputs is not None else tcm.scene_inputs(scene, cam, variant)
    leaf = {k: v.to(DEV).clone().requires_grad_(True) for k, v in inp.items() if k not in ("V", "campos")}
    st = _settings(scene, cam, W, H, garbage=cm is not None, debug=debug)
    if stats:
        P = leaf["means3D"].shape[0]
        kw["densify_stats"] = tuple(torch.zeros(P, device=DEV) for _ in range(3))
    model = {} if no_model else dict(camera_model=cm)
    features = kw.pop("features", None)
    call = dict(means3D=leaf["means3D"], means2D=leaf["means2D"], opacities=leaf["opacities"])
    call.update({NAMES[k]: v for k, v in leaf.items() if k in NAMES})
    if features is not None:
        call["features"] = features
    out = GaussianRasterizer(st, **model, **kw)(**call)
    grads = None
    if dL is not None:
        keys = ["image", None, "depth", "alpha"]
        loss = sum((out[i] * dL[k].to(DEV).reshape(out[i].shape)).sum() for i, k in enumerate(keys[:len(out)]) if k in dL)
        loss.backward()
        grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad).cpu().double() for k, v in leaf.items()}
        if stats:
            grads["densify_stats"] = tuple(t.cpu() for t in kw["densify_stats"])
    torch.cuda.synchronize()
    return tuple(o.detach().cpu() for o in out), grads


def reference(key, cm, scene, cam, W=None, H=None, variant="sh", maps=False, **kw):
    if key not in _REF:
        W, H = W or cam.image_width, H or cam.image_height
        shape = lambda st: {k: tcm.fragile_free(st, (c, H, W), seed) for k, c, seed in
                            ((("image", 3, 1), ("depth", 1, 2), ("alpha", 1, 3)) if maps else (("image", 3, 1),))}
        _REF[key] = tcm.reference(cm, W, H, scene.bg, 3, tcm.scene_inputs(scene, cam, variant), shape, **kw)
    return _REF[key]


def caps(st):
    assert float(st["fragile"].double().mean()) <= 0.10, "more than 10 % of the pixels are fragile"
    assert float(st["fragile_radius"].double().mean()) <= 0.01, "more than 1 % of the Gaussians have a fragile radius"


def check_radii(radii, want, st, what):
    bad = (radii.to(torch.int32) != want.to(torch.int32)) & ~st["fragile_radius"]
    assert not bool(bad.any()), (what, bad.nonzero().flatten().tolist()[:8])


def check_image(img, want, fragile, what):
    err = float(((img.double() - want.double()).abs() * (~fragile)).max())
    print(f"{what}: image error {err:.3e} (bar 1e-5)")
    util.parity_log(f"camera model {what}: image {err:.3e} / 1e-5")
    assert err <= 1e-5, (what, err)


def check_grads(g, want, d32, what, scale=None, chain=False):
    """chain: the wider band of the covariance chain's gradients (module docstring) -- test 4 only"""
    scale = scale or want
    miss = []
    for k in want:
        err = float((g[k] - want[k]).abs().max())
        bar = max(1e-5 * float(scale[k].abs().max()), 3.0 * d32[k])
        if chain and k in tcm.CHAIN:
            bar = max(bar, max(5e-5, 10.0 * d32["_split"][k]) * float(scale[k].abs().max()))
        print(f"{what}: {k} error {err:.3e} bar {bar:.3e} (max |g| {float(scale[k].abs().max()):.3e}, d32 {d32[k]:.3e})")
        util.parity_log(f"camera model {what}: {k} {err:.3e} / {bar:.3e}")
        if not err <= bar:
            miss.append((k, err, bar))
    assert not miss, (what, miss)


# ---- 1. default intrinsics reproduce the default path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", tcm.EDGE_SHAPES)
def test_default_intrinsics_reproduce_the_default_path(shape):
    W, H = shape
    scene, cam = tcm.base_scene(300, W, H)
    cm = tcm.default_model(W, H, cam.tanfovx, cam.tanfovy)
    out64, g64, d32, dL = reference(("default", shape), cm, scene, cam)
    st = out64["state"]
    caps(st)
    base, gb = hip(scene, cam, None, dL)
    out, g = hip(scene, cam, cm, dL)
    check_radii(out[1], base[1], st, f"default {shape}")
    check_image(out[0], base[0], st["fragile"], f"default {shape} vs the default path")
    check_grads(g, gb, d32, f"default {shape} vs the default path")
    # and both against the helper (the default path within the same bars: the helper is a valid reference of either)
    check_radii(out[1], st["radii"], st, f"default {shape} vs float64")
    check_image(out[0], out64["image"].detach(), st["fragile"], f"default {shape} vs float64")
    check_grads(g, g64, d32, f"default {shape} vs float64")


def test_none_is_the_default_path():
    """camera_model=None is bit-identical to omitting the keyword: image, radii, every gradient, densify_stats"""
    scene, cam = tcm.base_scene()
    dL = {"image": torch.randn(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(4))}
    a, ga = hip(scene, cam, None, dL, stats=True, no_model=True)
    b, gb = hip(scene, cam, None, dL, stats=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in ga:
        if k == "densify_stats":
            assert all(torch.equal(x, y) for x, y in zip(ga[k], gb[k])) and float(ga[k][1].sum()) > 0
        else:
            assert torch.equal(ga[k], gb[k]), k


# ---- 2. crop parity for the off-centre pinhole ---------------------------------------------------------------------------------------
def test_crop_parity_for_the_offcentre_pinhole():
    scene, cam, (W, H), (x0, y0), cm = tcm.crop_scene()
    BW, BH = cam.image_width, cam.image_height
    out64, g64, d32, dL = reference("crop", cm, scene, cam, W, H)
    st = out64["state"]
    caps(st)
    with torch.no_grad():
        inp = tcm.scene_inputs(scene, cam)
        big = tcm.render(tcm.default_model(BW, BH, cam.tanfovx, cam.tanfovy), BW, BH, scene.bg, 3, V=inp.pop("V"), campos=inp.pop("campos"), **inp)["state"]
    vis = st["vis"]
    assert bool(st["in_band"][vis].all()) and bool(big["in_band"][vis].all()), "a Gaussian of the crop sits in a guard band"
    fragile = st["fragile"] | big["fragile"][y0:y0 + H, x0:x0 + W]
    assert float(fragile.double().mean()) <= 0.10
    dcrop = dL["image"] * (~fragile).float()
    dbig = torch.zeros(3, BH, BW)
    dbig[:, y0:y0 + H, x0:x0 + W] = dcrop
    full, gf = hip(scene, cam, None, {"image": dbig})
    out, g = hip(scene, cam, cm, {"image": dcrop}, W=W, H=H)
    fr = st["fragile_radius"] | big["fragile_radius"]
    assert float(fr.double().mean()) <= 0.01
    bad = vis & ~fr & (out[1] != full[1])
    assert not bool(bad.any()), bad.nonzero().flatten().tolist()[:8]
    check_image(out[0], full[0][:, y0:y0 + H, x0:x0 + W], fragile, "crop vs the centred render")
    # means2D.grad is in NDC units of each image: 0.5 W dL/du -- compared per pixel unit
    gf["means2D"] = gf["means2D"] * torch.tensor([W / BW, H / BH, 1.0], dtype=torch.float64)
    check_grads(g, gf, d32, "crop vs the centred render")


# ---- 3. the asymmetric guard band ------------------------------------------------------------------------------------------------------
def test_asymmetric_guard_band():
    scene, cam, cm, k = tcm.guard_scene()
    W, H = cam.image_width, cam.image_height
    out64, g64, d32, dL = reference("guard", cm, scene, cam)
    st = out64["state"]
    caps(st)
    txtz = st["t"][:, 0] / st["t"][:, 2]
    between = st["vis"] & (txtz > 1.3 * cam.tanfovx) & (txtz < tcm.band(cm[1], cm[3], W)[1])
    assert int(between.sum()) >= 5 and bool(between[k].all())
    out, g = hip(scene, cam, cm, dL)
    check_radii(out[1], st["radii"], st, "guard band")
    check_image(out[0], out64["image"].detach(), st["fragile"], "guard band vs float64")
    check_grads(g, g64, d32, "guard band vs float64")
    # their means3D gradient through the covariance is there: far above the bar in the reference, so a kernel that zeroed it
    # (the symmetric band's x_grad_mul) could not have passed
    _, gcov = tcm.loss_and_grads(cm, W, H, scene.bg, 3, tcm.scene_inputs(scene, cam), dL, torch.float64, st, detach_pix=True)
    bar = max(1e-5 * float(g64["means3D"].abs().max()), 3.0 * d32["means3D"])
    strong = between & (gcov["means3D"][:, 0].abs() > 100.0 * bar)
    print(f"guard band: {int(strong.sum())} of {int(between.sum())} Gaussians with |dL/dx through the covariance| > 100 bars")
    assert int(strong.sum()) >= 5
    assert bool((g["means3D"][strong, 0] != 0).all())


# ---- 4. float64 autograd parity, both models -------------------------------------------------------------------------------------------
def _leaf_tensors(scene):
    """the optimiser's leaves of a scene: logits, log-scales, unnormalised quaternions, split SH"""
    op = scene.opacities.double().clamp(1e-4, 1 - 1e-4)
    g = torch.Generator().manual_seed(8)
    return dict(means3D=scene.means3D, means2D=torch.zeros_like(scene.means3D), features_dc=scene.shs[:, :1].contiguous(),
                features_rest=scene.shs[:, 1:].contiguous(), opacity=torch.log(op / (1 - op)).float(), scaling=torch.log(scene.scales),
                rotation=scene.rotations * (0.5 + torch.rand(scene.rotations.shape[0], 1, generator=g)))


def _leaf_reference(cm, W, H, scene, cam, leaves, dL, dtype, state):
    diff = {k: v.to(dtype).clone().requires_grad_(True) for k, v in leaves.items()}
    out = tcm.render(cm, W, H, scene.bg, 3, means3D=diff["means3D"], means2D=diff["means2D"], opacities=torch.sigmoid(diff["opacity"]),
                     scales=torch.exp(diff["scaling"]), rotations=torch.nn.functional.normalize(diff["rotation"], dim=1),
                     shs=torch.cat((diff["features_dc"], diff["features_rest"]), 1), V=cam.world_view_transform, campos=cam.camera_center,
                     dtype=dtype, state=state)
    loss = sum((out[k] * g.to(dtype).reshape(out[k].shape)).sum() for k, g in dL.items())
    grads = torch.autograd.grad(loss, list(diff.values()))
    return out, {k: g.detach().double() for k, g in zip(diff, grads)}


MODELS = {"pinhole": tcm.PINHOLE_OFFCENTRE, "fisheye": tcm.FISHEYE}


@pytest.mark.parametrize("variant", ["sh", "colors", "cov", "antialiasing", "depth", "invdepth"])
@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
def test_float64_autograd_parity(model, variant):
    scene, cam, _ = tcm.fisheye_scene()
    cm = MODELS[model]
    inputs = variant if variant in ("colors", "cov") else "sh"
    kw = dict(antialiasing=True) if variant == "antialiasing" else {}
    maps = variant in ("depth", "invdepth")
    ref_kw = dict(kw, depth_mode=variant) if maps else kw
    out64, g64, d32, dL = reference((model, variant), cm, scene, cam, variant=inputs, maps=maps, **ref_kw)
    st = out64["state"]
    caps(st)
    if model == "fisheye":
        r = st["t"][:, :2].norm(dim=1)
        assert bool(st["vis"][24]) and float(r[24]) == 0.0 and bool(st["vis"][25]) and float((r[25] / st["t"][25, 2]) ** 2) < tcm.SERIES_Q
        assert bool(st["vis"][26]) and float(torch.atan2(r[26], st["t"][26, 2])) > math.radians(75.0) and int((~st["vis"]).sum()) >= 10
    out, g = hip(scene, cam, cm, dL, variant=inputs, **(dict(depth_alpha=variant) if maps else {}), **kw)
    what = f"{model} {variant}"
    check_radii(out[1], st["radii"], st, what)
    check_image(out[0], out64["image"].detach(), st["fragile"], what)
    if maps:
        for i, k in ((2, "depth"), (3, "alpha")):
            err = float(((out[i][0].double() - out64[k].detach()).abs() * (~st["fragile"])).max())
            bar = 1e-5 * max(1.0, float(out64[k].detach().abs().max()))
            print(f"{what}: {k} map error {err:.3e} bar {bar:.3e}")
            assert err <= bar, (what, k, err)
    check_grads(g, g64, d32, what, chain=True)


@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
def test_float64_autograd_parity_leaf_mode(model):
    import fused_params
    scene, cam, _ = tcm.fisheye_scene()
    cm = MODELS[model]
    W, H = cam.image_width, cam.image_height
    leaves = _leaf_tensors(scene)
    scene_n = scene._replace(rotations=torch.nn.functional.normalize(leaves["rotation"], dim=1),
                             opacities=torch.sigmoid(leaves["opacity"]), scales=torch.exp(leaves["scaling"]))
    with torch.no_grad():
        inp = tcm.scene_inputs(scene_n, cam)
        st = tcm.render(cm, W, H, scene.bg, 3, V=inp.pop("V"), campos=inp.pop("campos"), **inp)["state"]
    caps(st)
    dL = {"image": tcm.fragile_free(st, (3, H, W))}
    out64, g64 = _leaf_reference(cm, W, H, scene, cam, leaves, dL, torch.float64, st)
    _, g32 = _leaf_reference(cm, W, H, scene, cam, leaves, dL, torch.float32, st)
    d32 = {k: float((g32[k] - g64[k]).abs().max()) for k in g64}
    d32["_split"] = tcm.split_sample(lambda d: _leaf_reference(cm, W, H, scene, cam, leaves, d, torch.float32, st)[1], dL, g32)
    t = {k: v.to(DEV).clone().requires_grad_(True) for k, v in leaves.items()}
    out = fused_params.rasterize_leaf_gaussians(t["means3D"], t["means2D"], t["features_dc"], t["features_rest"], t["opacity"], t["scaling"],
                                                t["rotation"], _settings(scene, cam, W, H, garbage=True), camera_model=cm)
    (out[0] * dL["image"].to(DEV)).sum().backward()
    g = {k: v.grad.cpu().double() for k, v in t.items()}
    what = f"{model} leaf mode"
    check_radii(out[1].cpu(), st["radii"], st, what)
    check_image(out[0].detach().cpu(), out64["image"].detach(), st["fragile"], what)
    check_grads(g, g64, d32, what, chain=True)


# ---- 5. the oracle pin, by composition ---------------------------------------------------------------------------------------------------
def test_fisheye_equals_the_oracle_on_pinhole_standins():
    """The unchanged CPU oracle renders, for every Gaussian, the centred-pinhole stand-in of its fisheye splat (same pixel mean, same
    2D covariance, same view depth; tcm.pinhole_standin): the fisheye image of the HIP path must be the oracle's."""
    scene, cam, cm = tcm.oracle_pin_scene()
    W, H = cam.image_width, cam.image_height
    inp = tcm.scene_inputs(scene, cam, "colors")
    with torch.no_grad():
        st = tcm.render(cm, W, H, scene.bg, 3, **inp)["state"]
    caps(st)
    S = tcm.covariance3d(scene.scales.double(), scene.rotations.double(), 1.0, None)
    mw, cov6, in_core = tcm.pinhole_standin(cm, W, H, cam.tanfovx, cam.tanfovy, scene.means3D, cam.world_view_transform, S)
    assert bool(in_core[st["vis"]].all()), "a visible stand-in sits in the oracle's guard band"
    o = util.oracle_forward(scene._replace(means3D=mw.float()), cam, 3, colors_precomp=inp["colors_precomp"], cov3D_precomp=cov6.float(),
                            use_sh=False, use_scale_rot=False)
    out, _ = hip(scene, cam, cm, variant="colors")
    fragile = torch.from_numpy(o["fragile"].reshape(H, W) != 0)
    assert float(fragile.double().mean()) <= 0.10
    check_image(out[0], torch.from_numpy(o["color"].reshape(3, H, W)), fragile, "fisheye vs the oracle's stand-ins")
    check_radii(out[1], torch.from_numpy(o["radii"].astype(np.int32)), st, "fisheye vs the oracle's stand-ins")


# ---- 6. edges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257])
def test_small_scenes(P):
    import gsr_scene
    scene, cam = gsr_scene.make_scene(P, -2.0, sh_degree=3, seed=P), gsr_scene.make_camera(37, 21)
    cm = ("fisheye", 13.0, 13.5, 18.2, 10.9)
    out64, g64, d32, dL = reference(("small", P), cm, scene, cam)
    st = out64["state"]
    caps(st)
    out, g = hip(scene, cam, cm, dL)
    bad = (out[1] != st["radii"]) & ~st["fragile_radius"]
    assert not bool(bad.any())
    check_image(out[0], out64["image"].detach(), st["fragile"], f"P = {P}")
    check_grads(g, g64, d32, f"P = {P}")


@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
def test_all_culled_scene_gives_exact_zeros(model):
    scene, cam = tcm.base_scene(130)
    means = scene.means3D.clone()
    means[:, 2] = -6.0 - means[:, 2].abs()          # behind the camera
    if model == "pinhole":
        means[100:, 2], means[100:, 1] = 0.0, 60.0  # in front, far off the image
    else:
        means[100:, 2] = -3.9                       # in front, inside the near plane (view z = 0.1 <= 0.2): this fisheye's image holds
                                                    # every direction of the half space, so nothing in front of it is off the image
    scene = scene._replace(means3D=means, scales=scene.scales.clamp(max=0.05))
    dL = {"image": torch.randn(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(2))}
    out, g = hip(scene, cam, MODELS[model], dL, stats=True)
    assert int(out[1].abs().sum()) == 0
    assert torch.equal(out[0], scene.bg[:, None, None].expand_as(out[0]))
    for k, v in g.items():
        if k == "densify_stats":
            assert all(float(t.abs().sum()) == 0.0 for t in v)
        else:
            assert float(v.abs().max()) == 0.0 and not bool(torch.isnan(v).any()), k


def test_only_the_last_lane_of_the_last_wave_is_visible():
    scene, cam = tcm.base_scene(320)    # five full waves: Gaussian 319 is lane 63 of the last one
    means = scene.means3D.clone()
    means[:, 2] = -6.0
    means[319] = torch.tensor([0.2, -0.1, 0.0])
    scene = scene._replace(means3D=means)
    cm = tcm.FISHEYE
    out64, g64, d32, dL = reference("lastlane", cm, scene, cam)
    st = out64["state"]
    caps(st)
    assert st["vis"].nonzero().flatten().tolist() == [319]
    out, g = hip(scene, cam, cm, dL)
    assert out[1].nonzero().flatten().tolist() == [319]
    check_image(out[0], out64["image"].detach(), st["fragile"], "last lane")
    check_grads(g, g64, d32, "last lane")
    for k, v in g.items():
        assert float(v[:319].abs().max()) == 0.0, k


@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
def test_bitwise_reproducible_and_independent_of_the_binning_path(model):
    from diff_gaussian_rasterization import _C
    scene, cam, _ = tcm.fisheye_scene()
    cm = MODELS[model]
    dL = {"image": torch.randn(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(6))}
    a, ga = hip(scene, cam, cm, dL, stats=True)
    b, gb = hip(scene, cam, cm, dL, stats=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in ga:
        if k == "densify_stats":
            assert all(torch.equal(x, y) for x, y in zip(ga[k], gb[k]))
        else:
            assert torch.equal(ga[k], gb[k]), k
    for bit in (_C.DEBUG_NO_TRIM, _C.DEBUG_TILE_SORT, _C.DEBUG_RADIX_DEPTH):
        c, _ = hip(scene, cam, cm, debug=bit)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]), bit


# ---- 7. everything downstream still composes -------------------------------------------------------------------------------------------
def test_every_downstream_feature_composes_with_the_fisheye():
    scene, cam, cm = tcm.fisheye_scene()
    W, H = cam.image_width, cam.image_height
    P = scene.means3D.shape[0]
    gen = torch.Generator().manual_seed(12)
    dL = {"image": torch.randn(3, H, W, generator=gen), "depth": torch.randn(1, H, W, generator=gen), "alpha": torch.randn(1, H, W, generator=gen)}
    plain, _ = hip(scene, cam, cm, variant="colors")
    inp = tcm.scene_inputs(scene, cam, "colors")
    feats = torch.cat((inp["colors_precomp"], torch.rand(P, 2, generator=gen)), 1).to(DEV).requires_grad_(True)   # K = 5
    absgrad = (torch.zeros(P, 2, device=DEV), torch.zeros(P, device=DEV))
    contrib = (torch.zeros(P, device=DEV), torch.zeros(P, device=DEV), torch.zeros(P, dtype=torch.int32, device=DEV))
    index_maps = (torch.zeros(H, W, dtype=torch.int32, device=DEV), torch.zeros(H, W, dtype=torch.int32, device=DEV), torch.zeros(H, W, device=DEV))
    from diff_gaussian_rasterization import GaussianRasterizer
    leaf = {k: v.to(DEV).clone().requires_grad_(True) for k, v in inp.items() if k not in ("V", "campos")}
    r = GaussianRasterizer(_settings(scene, cam, W, H, garbage=True), depth_alpha="depth", distortion=True, median_depth=True, absgrad=absgrad,
                           contrib_stats=contrib, index_maps=index_maps, camera_model=cm)
    color, radii, depth, alpha, dist, median, fmap = r(means3D=leaf["means3D"], means2D=leaf["means2D"], opacities=leaf["opacities"],
                                                       colors_precomp=leaf["colors_precomp"], scales=leaf["scales"],
                                                       rotations=leaf["rotations"], features=feats)
    loss = (color * dL["image"].to(DEV)).sum() + (depth * dL["depth"].to(DEV)).sum() + (alpha * dL["alpha"].to(DEV)).sum() + \
        dist.sum() + median.sum() + (fmap * fmap).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(color.detach().cpu(), plain[0]) and torch.equal(radii.cpu(), plain[1])
    bg = scene.bg[:, None, None]
    want = plain[0] - bg * (1.0 - alpha.detach().cpu())       # the colour image minus its background term
    assert float((fmap[:3].detach().cpu() - want).abs().max()) <= 1e-6
    for t in (leaf["means3D"].grad, leaf["scales"].grad, leaf["rotations"].grad, leaf["opacities"].grad, feats.grad, leaf["means2D"].grad):
        assert t is not None and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0
    assert float(absgrad[0].abs().max()) > 0 and float(contrib[0].max()) > 0 and int(index_maps[0].max()) >= 0
    assert tuple(depth.shape) == (1, H, W) and tuple(median.shape) == (1, H, W) and tuple(dist.shape) == (1, H, W)
