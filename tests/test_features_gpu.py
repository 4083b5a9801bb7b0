"""GPU: K per-Gaussian feature channels blended by the colour pass's own weights, with gradients to the features and to the geometry
(GaussianRasterizer.forward(features=...), rasterize_leaf_gaussians(features=...), include/gsr_features.h, csrc/features.hip).

The reference of the forward and of check_grads is the multi-pass composition a user had before: the image pass plus ceil(K / 3)
passes with colors_precomp = three feature channels and a zero background, through the existing rasterizer.  All passes take the HIP
kernels' decisions from the same bits, so the forward is compared bit for bit and no pixel is excluded anywhere.  Gradient bars are
test_depth_alpha_gpu.py's: 1e-5 of the reference's largest element, and for the scale / quaternion chain max(5e-5, 10 x the
split-composition band sample) measured per case.  A float64 autograd restatement (tests/torch_splat_feat.py) pins the hand-written
backward independently on a small scene, with the bars of tests/test_autograd_cpu.py."""
import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
import gsr_scene
import util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("means3D", "means2D", "shs", "opacities", "scales", "rotations")
CHAIN = ("scales", "rotations", "scaling", "rotation")
_cache = {}


def _scene(name):
    if name not in _cache:
        if name == "A":     # a one-pixel tile column and row, one list >= 1024: many batches, band-split forward, depth segments in the colour backward
            _cache[name] = (gsr_scene.make_scene(2000, -3.0, sh_degree=1, seed=33), gsr_scene.make_camera(33, 17), 1)
        elif name == "B":
            _cache[name] = (gsr_scene.make_scene(3000, -3.0, sh_degree=1, seed=21), gsr_scene.make_camera(120, 90), 1)
        else:
            from test_boundary_gpu import _heavy_scene
            _cache[name] = _heavy_scene()
    return _cache[name]


def _feats(P, K, seed=41):
    return torch.randn(P, K, generator=torch.Generator().manual_seed(seed))   # both signs


def _ups(K, H, W, seed=43):
    """upstream gradients: dL/dpix (3,H,W), dL/dfeature_map (K,H,W), dL/dD (1,H,W), dL/dA (1,H,W)"""
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(c, H, W, generator=g).to(DEV) for c in (3, K, 1, 1))


def _leaves(scene):
    t = {k: getattr(scene, k).to(DEV).clone().requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    t["means2D"] = torch.zeros(scene.means3D.shape, device=DEV, requires_grad=True)
    return t


def _grads(t, names):
    return {n: (t[n].grad.clone() if t[n].grad is not None else torch.zeros_like(t[n])) for n in names}


def _cam_settings(st, camera_grads):
    if not camera_grads:
        return st, ()
    cams = tuple(t.clone().requires_grad_(True) for t in (st.viewmatrix, st.projmatrix, st.campos))
    return st._replace(viewmatrix=cams[0], projmatrix=cams[1], campos=cams[2]), cams


def fused(scene, cam, D, feats, ups, *, debug=False, use_color=True, use_feat=True, antialiasing=False, depth_alpha=None,
          camera_grads=False, absgrad=None, densify_stats=None, backward=True):
    """One GaussianRasterizer call with features= -> dict(color, radii, fmap, [depth, alpha], grads incl. "features" [and "V", "PM",
    "campos"])."""
    from diff_gaussian_rasterization import GaussianRasterizer
    st, cams = _cam_settings(util.hip_settings(scene, cam, D, DEV, debug=debug), camera_grads)
    t = _leaves(scene)
    f = feats.to(DEV).clone().requires_grad_(True)
    kw = dict(camera_grads=True) if camera_grads else {}
    out = GaussianRasterizer(st, antialiasing=antialiasing, depth_alpha=depth_alpha, absgrad=absgrad, densify_stats=densify_stats, **kw)(
        **t, features=f)
    r = dict(color=out[0].detach(), radii=out[1], fmap=out[-1].detach())
    assert len(out) == (5 if depth_alpha else 3) and out[-1].shape == (feats.shape[1], cam.image_height, cam.image_width)
    if depth_alpha:
        r["depth"], r["alpha"] = out[2].detach(), out[3].detach()
    if backward:
        dpix, g, dD, dA = ups
        loss = 0
        if use_color:
            loss = loss + (out[0] * dpix).sum()
        if use_feat:
            loss = loss + (out[-1] * g).sum()
        if depth_alpha:
            loss = loss + (out[2] * dD).sum() + (out[3] * dA).sum()
        loss.backward()
        torch.cuda.synchronize()
        r["grads"] = _grads(t, NAMES)
        r["grads"]["features"] = f.grad.clone() if f.grad is not None else None
        for n, c in zip(("V", "PM", "campos"), cams):
            r["grads"][n] = c.grad.clone()
    return r


def composition(scene, cam, D, feats, ups, *, split=False, split_seed=99, antialiasing=False, depth_alpha=None, camera_grads=False):
    """The image pass plus ceil(K / 3) colors_precomp passes with a zero background; loss sum(color dpix) + sum(feature_map g)
    [+ the maps' terms].  split: the image pass's dL/dpix cut into two random parts, each with a pass of its own -- check_grads'
    reproducibility band (test_depth_alpha_gpu.two_pass).  -> dict(color, radii, fmap, grads)"""
    from diff_gaussian_rasterization import GaussianRasterizer
    st, cams = _cam_settings(util.hip_settings(scene, cam, D, DEV), camera_grads)
    st0 = st._replace(bg=torch.zeros(3, device=DEV))
    kw = dict(camera_grads=True) if camera_grads else {}
    t = _leaves(scene)
    f = feats.to(DEV).clone().requires_grad_(True)
    dpix, g, dD, dA = ups
    K = feats.shape[1]
    geo = {k: t[k] for k in ("means3D", "means2D", "opacities", "scales", "rotations")}
    out = GaussianRasterizer(st, antialiasing=antialiasing, depth_alpha=depth_alpha, **kw)(shs=t["shs"], **geo)
    if split:
        part = torch.randn(dpix.shape, generator=torch.Generator().manual_seed(split_seed)).to(DEV)
        c2 = GaussianRasterizer(st, antialiasing=antialiasing, **kw)(shs=t["shs"], **geo)[0]
        loss = (out[0] * part).sum() + (c2 * (dpix - part)).sum()
    else:
        loss = (out[0] * dpix).sum()
    if depth_alpha:
        loss = loss + (out[2] * dD).sum() + (out[3] * dA).sum()
    maps = []
    for k0 in range(0, K, 3):
        n = min(3, K - k0)
        cols = torch.cat([f[:, k0:k0 + n], torch.zeros(f.shape[0], 3 - n, device=DEV)], 1)
        m = GaussianRasterizer(st0, antialiasing=antialiasing, **kw)(colors_precomp=cols, **geo)[0]
        maps.append(m[:n])
    fmap = torch.cat(maps, 0)
    (loss + (fmap * g).sum()).backward()
    torch.cuda.synchronize()
    r = dict(color=out[0].detach(), radii=out[1], fmap=fmap.detach(), grads=_grads(t, NAMES))
    r["grads"]["features"] = f.grad.clone()
    for n, c in zip(("V", "PM", "campos"), cams):
        r["grads"][n] = c.grad.clone()
    return r


def _nerr(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-30)


def check_grads(g, rg, bands, label, names=NAMES + ("features",)):
    """test_depth_alpha_gpu.check_grads with dL/dfeatures among the 1e-5 tensors: 1e-5 of the reference's largest element for every
    tensor but the scale / quaternion chain; there max(5e-5, 10 x the band), the band being the reference side's own distance between
    two exact compositions (split=True), the largest of the samples in `bands`."""
    for n in names:
        e = _nerr(g[n], rg[n])
        b = max(5e-5, 10.0 * max(_nerr(band[n], rg[n]) for band in bands)) if n in CHAIN else 1e-5
        line = f"features {label} dL/d{n}: err {e:.2e} bar {b:.2e}"
        print(line)
        util.parity_log(line)
        assert e <= b, (label, n, e, b)


def _ranges(scene, cam, D, debug=0):
    from diff_gaussian_rasterization import _C
    r = _state(scene, cam, D, debug)
    W, H = cam.image_width, cam.image_height
    T = ((W + 15) // 16) * ((H + 15) // 16)
    il = _C.image_layout(W, H)
    return r[5][il.ranges:il.ranges + 8 * T].view(torch.int32).view(T, 2)


def _state(scene, cam, D, debug=0, colors=None, bg=None):
    """_C.rasterize_gaussians on the scene (SH colours, or colors_precomp = colors)."""
    from diff_gaussian_rasterization import _C
    st = util.hip_settings(scene, cam, D, DEV)
    e = torch.empty(0, device=DEV)
    t = {k: getattr(scene, k).to(DEV) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    r = _C.rasterize_gaussians(st.bg if bg is None else bg, t["means3D"], e if colors is None else colors, t["opacities"], t["scales"],
                               t["rotations"], 1.0, e, st.viewmatrix, st.projmatrix, st.tanfovx, st.tanfovy, st.image_height,
                               st.image_width, e if colors is not None else t["shs"], D, st.campos, False, debug)
    torch.cuda.synchronize()
    return r


# ---- 1. forward, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("K", [1, 4, 7])
def test_forward_equals_colour_passes_bit_for_bit(name, K):
    scene, cam, D = _scene(name)
    if name == "A":
        rng = _ranges(scene, cam, D)
        assert int((rng[:, 1] - rng[:, 0]).max()) >= 1024, "scene A no longer has a heavy tile"
        assert cam.image_width % 16 == 1 and cam.image_height % 16 == 1   # a one-pixel tile column and row
    feats = _feats(scene.means3D.shape[0], K)
    r = fused(scene, cam, D, feats, None, backward=False)
    f = feats.to(DEV)
    zero = torch.zeros(3, device=DEV)
    for k0 in range(0, K, 3):
        n = min(3, K - k0)
        cols = torch.cat([f[:, k0:k0 + n], torch.zeros(f.shape[0], 3 - n, device=DEV)], 1).contiguous()
        out_color = _state(scene, cam, D, colors=cols, bg=zero)[1]
        for c in range(n):
            assert torch.equal(r["fmap"][k0 + c], out_color[c]), (name, K, k0 + c)
    assert float(r["fmap"].abs().max()) > 0 and float(r["fmap"].min()) < 0 < float(r["fmap"].max())


# ---- 2. state and default path untouched ---------------------------------------------------------------------------------------------
def test_state_and_default_path_untouched():
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    scene, cam, D = _scene("A")
    P, W, H = scene.means3D.shape[0], cam.image_width, cam.image_height
    R, color, radii, geom, binning, img = _state(scene, cam, D)
    before = [b.clone() for b in (geom, binning, img)]
    fmap = _C.features_forward(geom, binning, img, R, P, W, H, _feats(P, 7).to(DEV))
    torch.cuda.synchronize()
    for a, b, n in zip(before, (geom, binning, img), ("geometry", "binning", "image")):
        assert torch.equal(a, b), f"gsr_features_forward wrote the {n} state"
    assert fmap.shape == (7, H, W)
    # colour and radii with features= are those without, and with the map left out of the loss so is every gradient
    ups = _ups(7, H, W)
    a = fused(scene, cam, D, _feats(P, 7), ups, use_feat=False)
    t = _leaves(scene)
    c, r = GaussianRasterizer(util.hip_settings(scene, cam, D, DEV))(**t)
    (c * ups[0]).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(a["color"], c.detach()) and torch.equal(a["radii"], r) and torch.equal(a["color"], color)
    g = _grads(t, NAMES)
    for n in NAMES:
        assert torch.equal(a["grads"][n], g[n]), n
    assert a["grads"]["features"] is None


# ---- 3. gradients against the multi-pass composition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "heavy"])
def test_gradients_match_the_multi_pass_composition(name):
    scene, cam, D = _scene(name)
    K = 7
    feats = _feats(scene.means3D.shape[0], K)
    ups = _ups(K, cam.image_height, cam.image_width)
    f = fused(scene, cam, D, feats, ups)
    r = composition(scene, cam, D, feats, ups)
    assert torch.equal(f["color"], r["color"]) and torch.equal(f["radii"], r["radii"]) and torch.equal(f["fmap"], r["fmap"])
    band = composition(scene, cam, D, feats, ups, split=True)["grads"]
    check_grads(f["grads"], r["grads"], [band], f"{name}/K={K}")


# ---- 4. independent of the hand-written formulas -------------------------------------------------------------------------------------
# The scene is chosen on the reference side alone: the fp32 CPU oracle's own composition of the same loss (its image pass plus two
# colour passes on a zero background, the arithmetic the kernels restate) sits at most 0.2 of every bar below away from the float64
# autograd result on it (means3D 1.8e-6, opacities 7.6e-7, shs 9.6e-7, scales 1.1e-6, rotations 1.4e-6, features 4.7e-7).  On
# make_scene(300, -2.6, seed=8) at the same size, for comparison, the oracle itself misses the rotations bar (1.3e-4: a needle-shaped
# splat), so no fp32 evaluation can be held to these bars there.  _check_small_scene_reference_side pins both properties.
SMALL = dict(P=250, mu=-2.4, seed=12, D=1, W=32, H=32, K=4)
# tests/test_autograd_cpu.py's bars for the same tensors; dL/dfeatures enters the blend exactly as a colour does -- linear in
# alpha T dL/dpix, no chain behind it -- and takes the bar of dL/dsh, the tensor with that position there
AUTOGRAD_BARS = dict(means3D=1.5e-5, opacities=5e-6, shs=5e-6, scales=6e-5, rotations=1e-4, features=5e-6)


def _small():
    if "small" not in _cache:
        s = SMALL
        scene = gsr_scene.make_scene(s["P"], s["mu"], sh_degree=s["D"], seed=s["seed"])
        scene = scene._replace(means3D=(scene.means3D * 0.6).contiguous())   # inside the frustum: the +-1.3 tan(fov) clamp inactive
        cam = gsr_scene.make_camera(s["W"], s["H"])
        o = util.oracle_forward(scene, cam, s["D"], margin=1e-3)
        _cache["small"] = (scene, cam, o)
    return _cache["small"]


def _small_loss():
    scene, cam, o = _small()
    s = SMALL
    ok = torch.from_numpy((o["fragile"] == 0).reshape(s["H"], s["W"]))
    g = torch.Generator().manual_seed(4)
    return _feats(s["P"], s["K"]), ok, torch.randn(3, s["H"], s["W"], generator=g) * ok, torch.randn(s["K"], s["H"], s["W"], generator=g) * ok


def _small_float64():
    """float64 autograd gradients of sum(image dpix) + sum(feature_map dmap) on the small scene, computed once"""
    if "small64" not in _cache:
        import torch_splat_feat
        scene, cam, o = _small()
        feats, ok, dpix, dmap = _small_loss()
        dt = torch.float64
        leaf = lambda t: t.to(dt).clone().requires_grad_(True)
        t = dict(means3D=leaf(scene.means3D), scales=leaf(scene.scales), rotations=leaf(scene.rotations), opacities=leaf(scene.opacities),
                 shs=leaf(scene.shs), features=leaf(feats))
        img, fmap = torch_splat_feat.render(o, t["means3D"], t["scales"], t["rotations"], t["opacities"], t["shs"], t["features"])
        ((img * dpix.to(dt)).sum() + (fmap * dmap.to(dt)).sum()).backward()
        _cache["small64"] = (img.detach(), fmap.detach(), {n: v.grad for n, v in t.items()})
    return _cache["small64"]


def _check_small_scene_reference_side():
    """On the CPU oracle's state alone (no device): the pixels whose accept / reject decisions sit within the oracle's margin are
    excluded from check 4 (as tests/test_autograd_cpu.py excludes them) and their share is capped at 5 %; and the fp32 oracle's own
    composition of the loss stays within half of every bar, so the bars can be asked of an fp32 evaluation on this scene."""
    from oracle import oracle
    scene, cam, o = _small()
    s = SMALL
    share = float((o["fragile"] != 0).mean())
    print(f"features small scene: fragile share {share:.4f}")
    assert share <= 0.05, share
    assert scene.means3D.shape[0] <= 300 and (cam.image_width, cam.image_height) == (32, 32) and s["K"] == 4
    feats, ok, dpix, dmap = _small_loss()
    og = oracle.backward(o, dpix.numpy())
    tot = {n: og[k].astype(np.float64).reshape(s["P"], -1) for n, k in (("means3D", "dL_dmeans3D"), ("opacities", "dL_dopacity"), ("shs", "dL_dsh"),
                                                                       ("scales", "dL_dscales"), ("rotations", "dL_drotations"))}
    tot["features"] = np.zeros((s["P"], s["K"]))
    black = scene._replace(bg=torch.zeros(3))
    for k0 in range(0, s["K"], 3):
        n = min(3, s["K"] - k0)
        cols = torch.cat([feats[:, k0:k0 + n], torch.zeros(s["P"], 3 - n)], 1).contiguous()
        oc = util.oracle_forward(black, cam, s["D"], margin=1e-3, colors_precomp=cols, use_sh=False)
        gc = oracle.backward(oc, torch.cat([dmap[k0:k0 + n], torch.zeros(3 - n, s["H"], s["W"])], 0).numpy())
        for nm, k in (("means3D", "dL_dmeans3D"), ("opacities", "dL_dopacity"), ("scales", "dL_dscales"), ("rotations", "dL_drotations")):
            tot[nm] += gc[k].astype(np.float64).reshape(s["P"], -1)
        tot["features"][:, k0:k0 + n] = gc["dL_dcolors"][:, :n]
    ref = _small_float64()[2]
    for n, bar in AUTOGRAD_BARS.items():
        b = ref[n].numpy().reshape(s["P"], -1)
        e = float(np.abs(tot[n] - b).max() / max(np.abs(b).max(), 1e-20))
        print(f"features small scene, oracle composition dL/d{n}: err {e:.2e} bar {bar:.2e}")
        assert e <= 0.5 * bar, (n, e, bar)


def test_gradients_match_float64_autograd():
    _check_small_scene_reference_side()
    scene, cam, o = _small()
    s = SMALL
    feats, ok, dpix, dmap = _small_loss()
    z = torch.zeros(1, s["H"], s["W"], device=DEV)
    f = fused(scene, cam, s["D"], feats, (dpix.to(DEV), dmap.to(DEV), z, z))
    img, fmap, ref = _small_float64()
    okn = ok.numpy()
    assert np.abs(img.numpy() - f["color"].cpu().numpy())[:, okn].max() < 5e-5
    assert np.abs(fmap.numpy() - f["fmap"].cpu().numpy())[:, okn].max() < 5e-5 * max(1.0, float(fmap.abs().max()))
    for n, bar in AUTOGRAD_BARS.items():
        a, b = f["grads"][n].cpu().double().reshape(s["P"], -1), ref[n].reshape(s["P"], -1)
        e = float((a - b).abs().max() / max(float(b.abs().max()), 1e-20))
        line = f"features float64 autograd dL/d{n}: err {e:.2e} bar {bar:.2e}"
        print(line)
        util.parity_log(line)
        assert e < bar, (n, e, bar)


# ---- 5. features-only mode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_features_only_mode(name):
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    scene, cam, D = _scene(name)
    P, K = scene.means3D.shape[0], 7
    feats = _feats(P, K)
    ups = _ups(K, cam.image_height, cam.image_width)
    full = fused(scene, cam, D, feats, ups)
    t = {k: getattr(scene, k).to(DEV) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    t["means2D"] = torch.zeros(P, 3, device=DEV)
    f = feats.to(DEV).clone().requires_grad_(True)
    calls = []
    orig = _C.backward_scratch
    _C.backward_scratch = lambda *a: (calls.append(a), orig(*a))[1]
    try:
        out = GaussianRasterizer(util.hip_settings(scene, cam, D, DEV))(**t, features=f)
        ((out[0] * ups[0]).sum() + (out[-1] * ups[1]).sum()).backward()
        torch.cuda.synchronize()
    finally:
        _C.backward_scratch = orig
    assert calls == [], "the features-only backward allocated the colour backward's scratch"
    assert torch.equal(f.grad, full["grads"]["features"])
    assert all(v.grad is None for v in t.values())
    assert float(f.grad.abs().max()) > 0


# ---- 6. variants ---------------------------------------------------------------------------------------------------------------------
def _variant(switches, K=4, names=NAMES + ("features",)):
    scene, cam, D = _scene("B")
    feats = _feats(scene.means3D.shape[0], K)
    ups = _ups(K, cam.image_height, cam.image_width)
    f = fused(scene, cam, D, feats, ups, **switches)
    r = composition(scene, cam, D, feats, ups, **switches)
    assert torch.equal(f["color"], r["color"]) and torch.equal(f["fmap"], r["fmap"])
    band = composition(scene, cam, D, feats, ups, split=True, **switches)["grads"]
    check_grads(f["grads"], r["grads"], [band], "B/" + ",".join(switches), names)
    return f, r, band


def test_variant_antialiasing():
    _variant(dict(antialiasing=True))


def test_variant_depth_alpha_with_both_map_gradients():
    _variant(dict(depth_alpha="depth"))


def test_variant_camera_grads():
    """The three camera tensors against the composition with camera_grads=True on every pass, with test_camera_grads_gpu.py's bar:
    max(1e-5 max sum_g |t_g|, 3 d32), t_g the Gaussians' own terms in float64 and d32 the float32 helper's distance from float64.
    At this size the terms take 20 s on the CPU, so sum_g |t_g| and d32 of this scene, these seeds and this loss are a fixture
    (tools/features_golden.py, tests/torch_splat_feat.camera_terms); the reference's totals must sit within the same bar of the
    fixture's float64 totals, which ties the fixture to the case."""
    import os
    K = 4
    f, r, _ = _variant(dict(camera_grads=True), K)
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "features_B_camera_terms.npz"))
    assert gold["scene"].tolist() == [3000, 1, 21, 120, 90, K, 41, 43], "the fixture belongs to another case: run tools/features_golden.py"
    for n in ("V", "PM", "campos"):
        bar = max(1e-5 * float(gold[f"abs_total_{n}"].max()), 3 * float(gold[f"d32_{n}"]))
        e = float((f["grads"][n].double() - r["grads"][n].double()).abs().max())
        tie = float((r["grads"][n].cpu().double().reshape(gold[f"total_{n}"].shape) - torch.from_numpy(gold[f"total_{n}"])).abs().max())
        line = f"features B/camera_grads dL/d{n}: err {e:.3e} bar {bar:.3e} (reference vs float64 {tie:.3e})"
        print(line)
        util.parity_log(line)
        assert e <= bar and tie <= bar, (n, e, tie, bar)


def test_camera_grads_against_float64_terms():
    """test_camera_grads_gpu.py's own scene, reference and bar, with a feature map in the loss."""
    import torch_splat_cam
    import torch_splat_feat
    scene, cam = torch_splat_cam.camera_test_scene()
    P, K, H, W = scene.means3D.shape[0], 4, cam.image_height, cam.image_width
    o = util.oracle_forward(scene, cam, 3)
    ok = torch.from_numpy((o["fragile"] == 0).reshape(H, W))
    assert float((~ok).float().mean()) < 0.05
    g = torch.Generator().manual_seed(3)
    dpix, dmap = torch.randn(3, H, W, generator=g) * ok, torch.randn(K, H, W, generator=g) * ok
    feats = _feats(P, K)
    inputs = dict(means3D=scene.means3D, opacities=scene.opacities, shs=scene.shs, scales=scene.scales, rotations=scene.rotations,
                  V=cam.world_view_transform, PM=cam.full_proj_transform, campos=cam.camera_center)
    total, abs_total, d32 = torch_splat_feat.camera_terms(o, inputs, feats, (dpix, dmap))
    z = torch.zeros(1, H, W, device=DEV)
    f = fused(scene, cam, 3, feats, (dpix.to(DEV), dmap.to(DEV), z, z), camera_grads=True)
    for k in ("V", "PM", "campos"):
        err = float((f["grads"][k].cpu().double().reshape(total[k].shape) - total[k]).abs().max())
        bar = max(1e-5 * float(abs_total[k].max()), 3 * d32[k])
        line = f"features camera scene dL/d{k}: err {err:.3e} bar {bar:.3e}"
        print(line)
        util.parity_log(line)
        assert err <= bar, (k, err, bar)


def test_variant_absgrad_is_the_colours_alone():
    scene, cam, D = _scene("B")
    P, K = scene.means3D.shape[0], 4
    feats = _feats(P, K)
    ups = _ups(K, cam.image_height, cam.image_width)
    mk = lambda: (torch.full((P, 2), 7.0, device=DEV), torch.zeros(P, device=DEV))
    a, b = mk(), mk()
    f = fused(scene, cam, D, feats, ups, absgrad=a)
    plain = fused(scene, cam, D, feats, ups, use_feat=False, absgrad=b)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(a[0].abs().max()) > 0
    assert not torch.equal(f["grads"]["means2D"], plain["grads"]["means2D"])
    r = composition(scene, cam, D, feats, ups)
    check_grads(f["grads"], r["grads"], [composition(scene, cam, D, feats, ups, split=True)["grads"]], "B/absgrad")


def test_variant_densify_stats_see_the_total_gradient():
    scene, cam, D = _scene("B")
    P, K = scene.means3D.shape[0], 4
    stats = tuple(torch.zeros(P, device=DEV) for _ in range(3))
    f = fused(scene, cam, D, _feats(P, K), _ups(K, cam.image_height, cam.image_width), densify_stats=stats)
    vis = f["radii"] > 0
    norm = torch.norm(f["grads"]["means2D"][:, :2], dim=-1) * vis
    assert torch.allclose(stats[0], norm, rtol=2e-6, atol=0)   # (test_renderer_gpu.py's bar for the same pair)
    assert torch.equal(stats[1], vis.float())
    plain = fused(scene, cam, D, _feats(P, K), _ups(K, cam.image_height, cam.image_width), use_feat=False)
    assert not torch.allclose(norm, torch.norm(plain["grads"]["means2D"][:, :2], dim=-1) * vis, rtol=1e-3, atol=0)


def test_variant_leaf_parameters():
    """rasterize_leaf_gaussians(features=) against the composition on the activated tensors (test_depth_alpha_gpu.test_leaf_parameters)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from fused_params import rasterize_leaf_gaussians
    from test_depth_alpha_gpu import LEAF_NAMES, _leaf_params
    scene, cam, D = _scene("B")
    P, K = scene.means3D.shape[0], 4
    feats = _feats(P, K)
    dpix, g, _, _ = _ups(K, cam.image_height, cam.image_width)
    lp = _leaf_params(scene)
    st = util.hip_settings(scene, cam, D, DEV)
    black = GaussianRasterizer(st._replace(bg=torch.zeros(3, device=DEV)))

    def leaves():
        t = {k: v.to(DEV).clone().requires_grad_(True) for k, v in lp.items()}
        t["means2D"] = torch.zeros(scene.means3D.shape, device=DEV, requires_grad=True)
        t["features"] = feats.to(DEV).clone().requires_grad_(True)
        return t

    def compose(u, split):
        act = dict(means3D=u["xyz"], means2D=u["means2D"], opacities=torch.sigmoid(u["opacity"]), scales=torch.exp(u["scaling"]),
                   rotations=torch.nn.functional.normalize(u["rotation"]))
        shs = torch.cat([u["features_dc"], u["features_rest"]], 1)
        c = GaussianRasterizer(st)(shs=shs, **act)[0]
        if split:
            part = torch.randn(dpix.shape, generator=torch.Generator().manual_seed(99)).to(DEV)
            loss = (c * part).sum() + (GaussianRasterizer(st)(shs=shs, **act)[0] * (dpix - part)).sum()
        else:
            loss = (c * dpix).sum()
        maps = []
        for k0 in range(0, K, 3):
            n = min(3, K - k0)
            cols = torch.cat([u["features"][:, k0:k0 + n], torch.zeros(P, 3 - n, device=DEV)], 1)
            maps.append(black(colors_precomp=cols, **act)[0][:n])
        fmap = torch.cat(maps, 0)
        (loss + (fmap * g).sum()).backward()
        torch.cuda.synchronize()
        return c.detach(), fmap.detach()

    names = LEAF_NAMES + ("features",)
    t = leaves()
    color, radii, fmap = rasterize_leaf_gaussians(t["xyz"], t["means2D"], t["features_dc"], t["features_rest"], t["opacity"], t["scaling"],
                                                  t["rotation"], st, features=t["features"])
    ((color * dpix).sum() + (fmap * g).sum()).backward()
    torch.cuda.synchronize()
    u, w = leaves(), leaves()
    rc, rf = compose(u, False)
    compose(w, True)
    assert torch.equal(color.detach(), rc) and torch.equal(fmap.detach(), rf)   # (as test_depth_alpha_gpu.check_forward: same bits)
    check_grads(_grads(t, names), _grads(u, names), [_grads(w, names)], "B/leaf", names)


# ---- 7. determinism and switches -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_determinism_and_debug_switches(name):
    from diff_gaussian_rasterization import _C
    scene, cam, D = _scene(name)
    K = 7
    feats = _feats(scene.means3D.shape[0], K)
    ups = _ups(K, cam.image_height, cam.image_width)
    a = fused(scene, cam, D, feats, ups)
    runs = [("second run", False), ("GSR_DEBUG_NO_CULL", _C.DEBUG_NO_CULL), ("GSR_DEBUG_NO_TRIM", _C.DEBUG_NO_TRIM)]
    if name == "A":
        runs.append(("GSR_DEBUG_NO_SPLIT", _C.DEBUG_NO_SPLIT))
    for label, debug in runs:
        b = fused(scene, cam, D, feats, ups, debug=debug)
        for k in ("color", "radii", "fmap"):
            assert torch.equal(a[k], b[k]), (name, label, k)
        for n in NAMES + ("features",):
            assert torch.equal(a["grads"][n], b["grads"][n]), (name, label, n)


# ---- 8. edges ------------------------------------------------------------------------------------------------------------------------
def test_edges():
    from diff_gaussian_rasterization import GaussianRasterizer
    # P = 0
    scene, cam, D = gsr_scene.make_scene(0, -3.0, sh_degree=0, seed=1), gsr_scene.make_camera(40, 30), 0
    r = fused(scene, cam, D, torch.zeros(0, 5), _ups(5, 30, 40))
    assert r["fmap"].shape == (5, 30, 40) and float(r["fmap"].abs().max()) == 0 and r["grads"]["features"].shape == (0, 5)
    # a scene behind the camera: nothing is rendered, the map and dL/dfeatures are zeros
    scene = gsr_scene.make_scene(500, -3.0, sh_degree=0, seed=2)
    scene = scene._replace(means3D=(scene.means3D * 0.01 - torch.tensor([0.0, 0.0, 20.0])).contiguous())
    r = fused(scene, cam, D, _feats(500, 5), _ups(5, 30, 40))
    assert int(r["radii"].abs().max()) == 0 and float(r["fmap"].abs().max()) == 0
    assert r["grads"]["features"].shape == (500, 5) and float(r["grads"]["features"].abs().max()) == 0
    only = fused(scene, cam, D, _feats(500, 5), _ups(5, 30, 40), use_color=False)
    assert float(only["grads"]["features"].abs().max()) == 0
    # one Gaussian, and K = 1 with a (P, 1) tensor
    scene = gsr_scene.make_scene(1, -1.0, sh_degree=0, seed=3)
    scene = scene._replace(means3D=torch.zeros(1, 3), opacities=torch.full((1, 1), 0.7))
    feats, ups = torch.tensor([[-1.5]]), _ups(1, 30, 40)
    r = fused(scene, cam, D, feats, ups)
    c = composition(scene, cam, D, feats, ups)
    assert torch.equal(r["fmap"], c["fmap"]) and float(r["fmap"].min()) < 0 and r["fmap"].shape == (1, 30, 40)
    check_grads(r["grads"], c["grads"], [composition(scene, cam, D, feats, ups, split=True)["grads"]], "one Gaussian/K=1")
    # under no_grad the map is returned and nothing is saved
    st = util.hip_settings(scene, cam, D, DEV)
    t = _leaves(scene)
    with torch.no_grad():
        out = GaussianRasterizer(st)(**t, features=feats.to(DEV).requires_grad_(True))
    assert torch.equal(out[-1], r["fmap"]) and all(o.grad_fn is None and not o.requires_grad for o in out)


def test_render_adds_features_on_both_paths():
    """render(..., features=) puts the map into the dict on the activated path and on the leaf path (pipe.fused_activations): the
    first has the bits of GaussianRasterizer(features=) on the model's activated tensors, the second agrees with it the way
    test_renderer_gpu.py's alternates agree (a rounding of an activation may flip a threshold)."""
    import gsr_model
    from diff_gaussian_rasterization import GaussianRasterizer
    from gaussian_renderer import render
    scene, cam, D = _scene("B")
    P, K = scene.means3D.shape[0], 4
    feats = _feats(P, K).to(DEV)
    camd = cam._replace(world_view_transform=cam.world_view_transform.to(DEV), full_proj_transform=cam.full_proj_transform.to(DEV),
                        camera_center=cam.camera_center.to(DEV))
    g = _ups(K, cam.image_height, cam.image_width)[1]
    for kw in ({}, dict(fused_activations=True)):
        pc = gsr_model.GaussianParams.from_activated(scene.means3D, scene.shs, scene.scales, scene.rotations, scene.opacities, device=DEV,
                                                     max_sh_degree=D, active_sh_degree=D)
        with torch.no_grad():
            ref = GaussianRasterizer(util.hip_settings(scene, cam, D, DEV))(
                means3D=pc.get_xyz, means2D=torch.zeros(P, 3, device=DEV), opacities=pc.get_opacity, shs=pc.get_features,
                scales=pc.get_scaling, rotations=pc.get_rotation, features=feats)
        f = feats.clone().requires_grad_(True)
        r = render(camd, pc, gsr_model.pipeline_params(**kw), scene.bg.to(DEV), features=f)
        assert set(r) == {"render", "viewspace_points", "visibility_filter", "radii", "features"}
        assert r["features"].shape == (K, cam.image_height, cam.image_width)
        if not kw:
            assert torch.equal(r["features"].detach(), ref[-1]) and torch.equal(r["render"].detach(), ref[0])
        else:
            d = (r["features"].detach() - ref[-1]).abs()
            assert float(d.mean()) < 1e-6 and float((d > 1e-4).float().mean()) < 1e-3, float(d.max())
        (r["features"] * g).sum().backward()
        assert f.grad is not None and float(f.grad.abs().max()) > 0 and float(r["viewspace_points"].grad.abs().max()) > 0
        assert "features" not in render(camd, pc, gsr_model.pipeline_params(**kw), scene.bg.to(DEV))
