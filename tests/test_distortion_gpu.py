"""GPU: the differentiable depth-distortion map Dist(p) = sum_{j<i} w_i w_j (v_i - v_j)^2 of a depth-and-alpha render
(GaussianRasterizer(depth_alpha=..., distortion=True), rasterize_leaf_gaussians(distortion=True), include/gsr_distortion.h,
csrc/distortion.hip).

References.  The forward is compared with the pairwise sum evaluated in float64 from weights the device itself produced: one-hot
`features=` channels give every w_i(p) with the forward's bits, the records give v_i.  Its tolerance is 10 x the distance of the
float32 restatement (tests/torch_splat_dist.py, dtype float32, centred at the mean v) from its float64 self on the same scene: a
different summation order is legitimate, a different precision class is not.  Gradients are compared with float64 autograd on a
small scene (tests/test_autograd_cpu.py's bars) and, at size, with a composition through the GPU's own feature path: features
(v - c, (v - c)^2, 1) with v computed in torch from means3D, Dist = A Q - D^2 formed in torch, so dL/dv reaches means3D by
autograd (bars of test_features_gpu.check_grads: 1e-5 of the largest element; scale / quaternion chain max(5e-5, 10 x the
split-composition band))."""
import math
import os

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
import gsr_scene
import util
from test_depth_alpha_gpu import _v
from test_features_gpu import NAMES, _cam_settings, _grads, _leaves, _nerr, _scene, check_grads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ("depth", "invdepth")
_cache = {}


def _ups(H, W, seed=47):
    """upstream gradients: dL/dpix (3,H,W), dL/dDist (1,H,W), dL/dD (1,H,W), dL/dA (1,H,W)"""
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(c, H, W, generator=g).to(DEV) for c in (3, 1, 1, 1))


def fused(scene, cam, D, mode, ups, *, debug=False, use_color=True, use_dist=True, use_maps=False, antialiasing=False,
          camera_grads=False, absgrad=None, densify_stats=None, features=None, dfeat=None, backward=True, distortion=True):
    """One GaussianRasterizer call -> dict(color, radii, depth, alpha, [dist], [fmap], grads [incl. "features", "V", "PM", "campos"])."""
    from diff_gaussian_rasterization import GaussianRasterizer
    st, cams = _cam_settings(util.hip_settings(scene, cam, D, DEV, debug=debug), camera_grads)
    t = _leaves(scene)
    kw = dict(camera_grads=True) if camera_grads else {}
    if distortion:
        kw["distortion"] = True
    f = None if features is None else features.to(DEV).clone().requires_grad_(True)
    fk = {} if f is None else dict(features=f)
    out = GaussianRasterizer(st, antialiasing=antialiasing, depth_alpha=mode, absgrad=absgrad, densify_stats=densify_stats, **kw)(**t, **fk)
    H, W = cam.image_height, cam.image_width
    assert len(out) == 4 + (1 if distortion else 0) + (0 if f is None else 1)
    r = dict(color=out[0].detach(), radii=out[1], depth=out[2].detach(), alpha=out[3].detach())
    if distortion:
        assert out[4].shape == (1, H, W)
        r["dist"] = out[4].detach()
    if f is not None:
        assert out[-1].shape == (features.shape[1], H, W)
        r["fmap"] = out[-1].detach()
    if backward:
        dpix, g, dD, dA = ups
        loss = 0
        if use_color:
            loss = loss + (out[0] * dpix).sum()
        if use_dist and distortion:
            loss = loss + (out[4] * g).sum()
        if use_maps:
            loss = loss + (out[2] * dD).sum() + (out[3] * dA).sum()
        if f is not None and dfeat is not None:
            loss = loss + (out[-1] * dfeat).sum()
        loss.backward()
        torch.cuda.synchronize()
        r["grads"] = _grads(t, NAMES)
        if f is not None:
            r["grads"]["features"] = None if f.grad is None else f.grad.clone()
        for n, c in zip(("V", "PM", "campos"), cams):
            r["grads"][n] = c.grad.clone()
    return r


def composition(scene, cam, D, mode, ups, *, split=False, use_color=True, use_maps=False, antialiasing=False, camera_grads=False,
                detach_v=False):
    """The same loss through the GPU's own feature path: features (v - c, (v - c)^2, 1) with v computed in torch from means3D (and
    the view matrix), Dist = A Q - D^2 formed in torch; autograd adds dL/dv from dL/dfeatures.  split: the image pass's dL/dpix cut
    into two random parts, each with a pass of its own (check_grads' band).  detach_v: the depths as constants (no z-axis term)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    st, cams = _cam_settings(util.hip_settings(scene, cam, D, DEV), camera_grads)
    kw = dict(camera_grads=True) if camera_grads else {}
    t = _leaves(scene)
    dpix, g, dD, dA = ups
    v = _v(t["means3D"], st.viewmatrix, mode)
    if detach_v:
        v = v.detach()
    u = v - float(v.detach().mean())
    feats = torch.stack([u, u * u, torch.ones_like(u)], 1)
    out = GaussianRasterizer(st, antialiasing=antialiasing, depth_alpha=mode, **kw)(**t, features=feats)
    m = out[-1]
    dist = (m[2] * m[1] - m[0] * m[0])[None]
    loss = (dist * g).sum()
    if use_color and split:
        part = torch.randn(dpix.shape, generator=torch.Generator().manual_seed(99)).to(DEV)
        c2 = GaussianRasterizer(st, antialiasing=antialiasing, **kw)(**t)[0]
        loss = loss + (out[0] * part).sum() + (c2 * (dpix - part)).sum()
    elif use_color:
        loss = loss + (out[0] * dpix).sum()
    if use_maps:
        loss = loss + (out[2] * dD).sum() + (out[3] * dA).sum()
    loss.backward()
    torch.cuda.synchronize()
    r = dict(color=out[0].detach(), radii=out[1], dist=dist.detach(), grads=_grads(t, NAMES))
    for n, c in zip(("V", "PM", "campos"), cams):
        r["grads"][n] = c.grad.clone()
    return r


def _direct(scene, cam, D, mode, debug=0, antialiasing=False):
    """_C.rasterize_gaussians_depth_alpha on the scene -> its nine results"""
    from diff_gaussian_rasterization import _C
    st = util.hip_settings(scene, cam, D, DEV)
    e = torch.empty(0, device=DEV)
    t = {k: getattr(scene, k).to(DEV) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    r = _C.rasterize_gaussians_depth_alpha(mode, st.bg, t["means3D"], e, t["opacities"], t["scales"], t["rotations"], 1.0, e, st.viewmatrix,
                                           st.projmatrix, st.tanfovx, st.tanfovy, st.image_height, st.image_width, t["shs"], D, st.campos,
                                           False, debug, antialiasing=antialiasing)
    torch.cuda.synchronize()
    return r


def _device_v(geom, radii):
    """the depth values the preprocess put into the splat records' last word; 0 for Gaussians without a record"""
    from diff_gaussian_rasterization import _C
    P = radii.shape[0]
    gl = _C.geometry_layout(P)
    v = geom[gl.splat:gl.splat + 48 * P].view(torch.float32).view(P, 12)[:, 11]
    return torch.where(radii > 0, v, torch.zeros_like(v))


def device_maps(scene, cam, D, mode, antialiasing=False):
    """-> (Dist of gsr_distortion_forward (H,W), the pairwise sum in float64 from the device's own weights (one-hot feature channels)
    and depth values (H,W), the fp32 raw-moment form A Q - D^2 from the device's own moment maps of (v, v^2, 1) (H,W))"""
    from diff_gaussian_rasterization import _C
    P, W, H = scene.means3D.shape[0], cam.image_width, cam.image_height
    R, color, radii, geom, binning, img, depth, alpha, auxbuf = _direct(scene, cam, D, mode, antialiasing=antialiasing)
    dist, state = _C.distortion_forward(geom, binning, img, R, P, W, H)
    v = _device_v(geom, radii)
    w = _C.features_forward(geom, binning, img, R, P, W, H, torch.eye(P, device=DEV)).reshape(P, H * W).double()   # w_i(p), the forward's bits
    u = (v - v[radii > 0].mean()).double() if bool((radii > 0).any()) else v.double()
    A, Dm, Q = w.sum(0), u @ w, (u * u) @ w
    pair = (A * Q - Dm * Dm).reshape(H, W)   # = sum_{j<i} w_i w_j (v_i - v_j)^2, exact enough in float64
    m = _C.features_forward(geom, binning, img, R, P, W, H, torch.stack([v, v * v, torch.ones_like(v)], 1).contiguous())
    raw = m[2] * m[1] - m[0] * m[0]
    torch.cuda.synchronize()
    # the state the backward reads is the map's own: Dist = A S, A = the sum of the weights
    assert torch.equal(dist[0], state[0] * state[2])
    assert float((state[0].double() - A.reshape(H, W)).abs().max()) < 1e-5
    return dist[0], pair, raw


def restatement(key, scene, cam, D, mode, margin=1e-3):
    """The float64 restatement's map and the float32 (centred) restatement's distance from it on the scene, computed once on the CPU
    -> (oracle state, ok mask (H,W), Dist64 (H,W), e32 = max |Dist32 - Dist64|)"""
    if (key, mode) not in _cache:
        import torch_splat_dist
        o = util.oracle_forward(scene, cam, D, margin=margin)
        ok = torch.from_numpy((o["fragile"] == 0).reshape(cam.image_height, cam.image_width))
        with torch.no_grad():
            d64, d32 = (torch_splat_dist.render(o, scene.means3D, scene.scales, scene.rotations, scene.opacities, scene.shs, mode,
                                                dtype=dt)[3].double() for dt in (torch.float64, torch.float32))
        _cache[(key, mode)] = (o, ok, d64, float((d32 - d64).abs().max()))
    return _cache[(key, mode)]


# ---- 1. the definition, on the device's own weights ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("mode", MODES)
def test_map_is_the_pairwise_sum_of_the_devices_own_weights(name, mode):
    from test_features_gpu import _ranges
    scene, cam, D = _scene(name)
    if name == "A":
        rng = _ranges(scene, cam, D)
        assert int((rng[:, 1] - rng[:, 0]).max()) >= 1024, "scene A no longer has a heavy tile"
        assert cam.image_width % 16 == 1 and cam.image_height % 16 == 1   # a one-pixel tile column and row
    dist, pair, _ = device_maps(scene, cam, D, mode)
    _, _, d64, e32 = restatement(name, scene, cam, D, mode)
    err = float((dist.double() - pair).abs().max())
    line = (f"distortion {name}/{mode}: device vs float64 pairwise sum of its own weights {err:.3e}; fp32 restatement vs float64 {e32:.3e} "
            f"(tolerance {10 * e32:.3e}); max Dist {float(pair.max()):.3e}")
    print(line)
    util.parity_log(line)
    assert float(pair.max()) > 0 and float(pair.min()) > -1e-12
    assert float(dist.min()) >= 0.0
    assert err <= 10 * e32, (name, mode, err, e32)


# ---- 2. state and default path untouched -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_state_and_default_path_untouched(mode):
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    scene, cam, D = _scene("A")
    P, W, H = scene.means3D.shape[0], cam.image_width, cam.image_height
    R, color, radii, geom, binning, img, depth, alpha, auxbuf = _direct(scene, cam, D, mode)
    before = [b.clone() for b in (geom, binning, img, auxbuf, color, radii, depth, alpha)]
    dist, state = _C.distortion_forward(geom, binning, img, R, P, W, H)
    torch.cuda.synchronize()
    for a, b, n in zip(before, (geom, binning, img, auxbuf, color, radii, depth, alpha),
                       ("geometry", "binning", "image", "aux scratch", "colour", "radii", "depth", "alpha")):
        assert torch.equal(a, b), f"gsr_distortion_forward wrote the {n}"
    assert dist.shape == (1, H, W) and state.shape == (3, H, W) and float(dist.max()) > 0
    # the module: colour, radii, depth and alpha with distortion=True are those without; the map is the direct call's
    ups = _ups(H, W)
    a = fused(scene, cam, D, mode, ups, backward=False)
    b = fused(scene, cam, D, mode, ups, backward=False, distortion=False)
    for k in ("color", "radii", "depth", "alpha"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["color"], color) and torch.equal(a["depth"], depth) and torch.equal(a["dist"], dist)
    # the default call's outputs are what they were
    c, r = GaussianRasterizer(util.hip_settings(scene, cam, D, DEV))(**_leaves(scene))
    assert torch.equal(c.detach(), color) and torch.equal(r, radii)


# ---- 3. gradients against float64 autograd -----------------------------------------------------------------------------------------------
# tests/test_autograd_cpu.py's bars, relative to the largest element of each tensor
AUTOGRAD_BARS = dict(means3D=1.5e-5, opacities=5e-6, shs=5e-6, scales=6e-5, rotations=1e-4)
# the small scene of test_features_gpu.py's check 4 (250 Gaussians at 32 x 32, means scaled 0.6 into the frustum).  Measured on the
# reference side (fp32 restatement vs float64, both modes): means3D 1.6e-6, opacities 4.6e-7, shs 6.3e-7, scales 9.7e-7, rotations
# 1.5e-6; fragile share 0.39 %.


def _small_reference(mode):
    """-> (scene, cam, ok, dpix, g, Dist64, float64 gradients); the reference-side check runs here, with no device"""
    if ("small", mode) not in _cache:
        import torch_splat_dist
        from test_features_gpu import SMALL, _small
        scene, cam, o = _small()
        s = SMALL
        ok = torch.from_numpy((o["fragile"] == 0).reshape(s["H"], s["W"]))
        share = float((~ok).float().mean())
        print(f"distortion small scene: fragile share {share:.4f}")
        assert share <= 0.05, share
        gen = torch.Generator().manual_seed(4)
        dpix, g = torch.randn(3, s["H"], s["W"], generator=gen) * ok, torch.randn(1, s["H"], s["W"], generator=gen) * ok
        res = {}
        for dt in (torch.float64, torch.float32):
            leaf = lambda x: x.to(dt).clone().requires_grad_(True)
            t = dict(means3D=leaf(scene.means3D), scales=leaf(scene.scales), rotations=leaf(scene.rotations), opacities=leaf(scene.opacities),
                     shs=leaf(scene.shs))
            img, _, _, dist = torch_splat_dist.render(o, t["means3D"], t["scales"], t["rotations"], t["opacities"], t["shs"], mode, dtype=dt)
            ((img * dpix.to(dt)).sum() + (dist * g[0].to(dt)).sum()).backward()
            res[dt] = (dist.detach().double(), {n: v.grad.double() for n, v in t.items()})
        for n, bar in AUTOGRAD_BARS.items():   # the bars can be asked of an fp32 evaluation on this scene
            e = _nerr(res[torch.float32][1][n], res[torch.float64][1][n])
            print(f"distortion small scene/{mode}, fp32 restatement dL/d{n}: err {e:.2e} bar {bar:.2e}")
            assert e <= 0.5 * bar, (n, e, bar)
        _cache[("small", mode)] = (scene, cam, ok, dpix, g, res[torch.float64][0], res[torch.float64][1],
                                   float((res[torch.float32][0] - res[torch.float64][0]).abs().max()))
    return _cache[("small", mode)]


@pytest.mark.parametrize("mode", MODES)
def test_gradients_match_float64_autograd(mode):
    from test_features_gpu import SMALL
    scene, cam, ok, dpix, g, d64, ref, e32 = _small_reference(mode)
    z = torch.zeros(1, SMALL["H"], SMALL["W"], device=DEV)
    f = fused(scene, cam, SMALL["D"], mode, (dpix.to(DEV), g.to(DEV), z, z))
    err = float((f["dist"][0].cpu().double() - d64).abs()[ok].max())
    print(f"distortion small scene/{mode}: map vs float64 {err:.3e} (fp32 restatement {e32:.3e})")
    assert err <= 10 * e32, (err, e32)
    assert float((f["dist"][0].cpu() * ok).abs().max()) > 0
    for n, bar in AUTOGRAD_BARS.items():
        e = _nerr(f["grads"][n].cpu().reshape(ref[n].shape), ref[n])
        line = f"distortion float64 autograd/{mode} dL/d{n}: err {e:.2e} bar {bar:.2e}"
        print(line)
        util.parity_log(line)
        assert e < bar, (n, e, bar)


# ---- 4. conditioning ---------------------------------------------------------------------------------------------------------------------
def _far_camera(W=120, H=90, z=53.0):
    """scene B seen from z = -53 through a lens narrowed by the same factor: every depth is in [51.5, 54.5], the spread and the image
    are those of the near camera (up to perspective)"""
    return gsr_scene.make_camera(W, H, fovx=2.0 * math.atan(math.tan(0.5) * 4.0 / z), T=np.array([0.0, 0.0, z]))


def test_far_scene_keeps_its_digits():
    """Depths >= 50 with a spread of 3: the centred recurrence keeps the fp32 restatement's accuracy, the raw moments A Q - D^2
    (formed in fp32 from the device's own moment maps of v and v^2) lose about four digits and miss the tolerance."""
    scene, _, D = _scene("B")
    cam = _far_camera()
    dist, pair, raw = device_maps(scene, cam, D, "depth")
    o, ok, d64, e32 = restatement("far", scene, cam, D, "depth")
    assert float(o["depths"][o["radii"] > 0].min()) >= 50.0
    share = float((~ok).float().mean())
    assert share <= 0.05, share
    okd = ok.to(DEV)
    ref = d64.to(DEV)
    err = float((dist.double() - ref).abs()[okd].max())
    err_raw = float((raw.double() - ref).abs()[okd].max())
    err_pair = float((dist.double() - pair).abs().max())
    line = (f"distortion far B/depth: device vs float64 restatement {err:.3e}, vs its own pairwise sum {err_pair:.3e}; raw fp32 moments "
            f"{err_raw:.3e}; fp32 centred restatement {e32:.3e} (tolerance {10 * e32:.3e}); max Dist {float(ref.max()):.3e}; fragile {share:.4f}")
    print(line)
    util.parity_log(line)
    assert err <= 10 * e32 and err_pair <= 10 * e32, (err, err_pair, e32)
    assert err_raw > 10 * e32, "the raw-moment form was expected to miss the tolerance on this scene"


# ---- 5. variants on B --------------------------------------------------------------------------------------------------------------------
def _variant(switches, mode="depth", names=NAMES, **loss):
    scene, cam, D = _scene("B")
    ups = _ups(cam.image_height, cam.image_width)
    f = fused(scene, cam, D, mode, ups, **switches, **loss)
    r = composition(scene, cam, D, mode, ups, **switches, **loss)
    assert torch.equal(f["color"], r["color"]) and torch.equal(f["radii"], r["radii"])
    band = composition(scene, cam, D, mode, ups, split=True, **switches, **loss)["grads"]
    check_grads(f["grads"], r["grads"], [band], f"distortion B/{mode}/" + ",".join(list(switches) + list(loss)), names)
    return f, r


@pytest.mark.parametrize("mode", MODES)
def test_variant_plain_and_with_both_map_gradients(mode):
    _variant({}, mode)
    _variant({}, mode, use_maps=True)


def test_variant_antialiasing():
    scene, cam, D = _scene("B")
    f, _ = _variant(dict(antialiasing=True))
    dist, pair, _ = device_maps(scene, cam, D, "depth", antialiasing=True)
    assert torch.equal(f["dist"][0], dist)
    assert float((dist.double() - pair).abs().max()) <= 10 * restatement("B", scene, cam, D, "depth")[3]
    assert not torch.equal(dist, device_maps(scene, cam, D, "depth")[0])


def test_variant_only_the_distortion_gradient():
    """dL/dpix, dL/dD and dL/dA absent: the aux backward kernels still run, and dL/dmeans3D carries the z-axis term of dL/dv."""
    from diff_gaussian_rasterization import _C
    calls = []
    orig = _C.aux_backward_args
    _C.aux_backward_args = lambda *a: (calls.append(a[2:4]), orig(*a))[1]
    try:
        f, r = _variant({}, use_color=False)
    finally:
        _C.aux_backward_args = orig
    assert calls == [(None, None)], "the distortion gradient alone must take the aux backward, without map gradients"
    scene, cam, D = _scene("B")
    flat = composition(scene, cam, D, "depth", _ups(cam.image_height, cam.image_width), use_color=False, detach_v=True)
    assert _nerr(flat["grads"]["means3D"], r["grads"]["means3D"]) > 1e-3, "the z-axis term is too small to be seen on this scene"


def test_variant_camera_grads():
    """The three camera tensors against the float64 per-Gaussian terms of tests/torch_splat_dist.py, with test_camera_grads_gpu.py's
    bar: max(1e-5 max sum_g |t_g|, 3 d32).  At this size the terms take a minute on the CPU, so they are a fixture
    (tools/distortion_golden.py) -- of this scene, these seeds and this loss, on the pixels the oracle does not call fragile."""
    scene, cam, D = _scene("B")
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distortion_B_camera_terms.npz"))
    assert gold["scene"].tolist() == [3000, 1, 21, 120, 90, 47], "the fixture belongs to another case: run tools/distortion_golden.py"
    o, ok, _, _ = restatement("B", scene, cam, D, "depth", margin=float(gold["margin"]))
    assert np.array_equal(ok.numpy(), gold["ok"]) and float((~ok).float().mean()) <= 0.05
    dpix, g, dD, dA = _ups(cam.image_height, cam.image_width)
    okd = ok.to(DEV)
    f = fused(scene, cam, D, "depth", (dpix * okd, g * okd, dD, dA), camera_grads=True)
    for n in ("V", "PM", "campos"):
        total = torch.from_numpy(gold[f"total_{n}"])
        bar = max(1e-5 * float(gold[f"abs_total_{n}"].max()), 3 * float(gold[f"d32_{n}"]))
        e = float((f["grads"][n].cpu().double().reshape(total.shape) - total).abs().max())
        line = f"distortion B/camera_grads dL/d{n}: err {e:.3e} bar {bar:.3e}"
        print(line)
        util.parity_log(line)
        assert e <= bar, (n, e, bar)
    # ... and with the composition on the same passes, for the Gaussians' gradients with the camera kernels
    _variant(dict(camera_grads=True))


def test_variant_absgrad_is_the_colours_alone():
    scene, cam, D = _scene("B")
    P = scene.means3D.shape[0]
    ups = _ups(cam.image_height, cam.image_width)
    mk = lambda: (torch.full((P, 2), 7.0, device=DEV), torch.zeros(P, device=DEV))
    a, b = mk(), mk()
    f = fused(scene, cam, D, "depth", ups, use_maps=True, absgrad=a)
    plain = fused(scene, cam, D, "depth", ups, use_maps=True, use_dist=False, absgrad=b)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(a[0].abs().max()) > 0
    assert not torch.equal(f["grads"]["means2D"], plain["grads"]["means2D"])
    r = composition(scene, cam, D, "depth", ups, use_maps=True)
    check_grads(f["grads"], r["grads"], [composition(scene, cam, D, "depth", ups, use_maps=True, split=True)["grads"]], "distortion B/absgrad", NAMES)


def test_variant_densify_stats_see_the_total_gradient():
    scene, cam, D = _scene("B")
    P = scene.means3D.shape[0]
    ups = _ups(cam.image_height, cam.image_width)
    stats = tuple(torch.zeros(P, device=DEV) for _ in range(3))
    f = fused(scene, cam, D, "depth", ups, densify_stats=stats)
    vis = f["radii"] > 0
    norm = torch.norm(f["grads"]["means2D"][:, :2], dim=-1) * vis
    assert torch.allclose(stats[0], norm, rtol=2e-6, atol=0)   # (test_renderer_gpu.py's bar for the same pair)
    assert torch.equal(stats[1], vis.float())
    plain = fused(scene, cam, D, "depth", ups, use_dist=False)
    assert not torch.allclose(norm, torch.norm(plain["grads"]["means2D"][:, :2], dim=-1) * vis, rtol=1e-3, atol=0)


def test_variant_features_and_distortion_together():
    """(color, radii, depth, alpha, distortion, feature_map), and both gradients: the gradients of the sum of the two losses are the
    sum of the two runs' gradients (the slots add them before the per-Gaussian chain: check_grads' bars, the band being the chain's)."""
    scene, cam, D = _scene("B")
    P, K = scene.means3D.shape[0], 4
    H, W = cam.image_height, cam.image_width
    ups = _ups(H, W)
    feats = torch.randn(P, K, generator=torch.Generator().manual_seed(41))
    gf = torch.randn(K, H, W, generator=torch.Generator().manual_seed(43)).to(DEV)
    both = fused(scene, cam, D, "depth", ups, features=feats, dfeat=gf)
    d_only = fused(scene, cam, D, "depth", ups)
    f_only = fused(scene, cam, D, "depth", ups, features=feats, dfeat=gf, use_color=False, distortion=False)
    assert torch.equal(both["dist"], d_only["dist"]) and torch.equal(both["fmap"], f_only["fmap"])
    assert torch.equal(both["grads"]["features"], f_only["grads"]["features"]) and float(both["grads"]["features"].abs().max()) > 0
    total = {n: d_only["grads"][n] + f_only["grads"][n] for n in NAMES}
    band = composition(scene, cam, D, "depth", ups, split=True)["grads"]
    ref = composition(scene, cam, D, "depth", ups)["grads"]
    check_grads(both["grads"], total, [{n: band[n] - ref[n] + total[n] for n in NAMES}], "distortion B/features+distortion", NAMES)
    assert _nerr(both["grads"]["means3D"], d_only["grads"]["means3D"]) > 1e-3


def test_variant_no_gradient_on_the_map_runs_the_parents_backward():
    from diff_gaussian_rasterization import _C
    scene, cam, D = _scene("B")
    ups = _ups(cam.image_height, cam.image_width)
    runs, aux = [], []
    orig_run, orig_aux = _C.DistortionBackward.run, _C.aux_backward_args
    _C.DistortionBackward.run = lambda self, *a: (runs.append(1), orig_run(self, *a))[1]
    _C.aux_backward_args = lambda *a: (aux.append(1), orig_aux(*a))[1]
    try:
        a = fused(scene, cam, D, "depth", ups, use_dist=False, use_maps=True)
        b = fused(scene, cam, D, "depth", ups, use_maps=True, distortion=False)
        assert runs == [] and len(aux) == 2
        c = fused(scene, cam, D, "depth", ups, use_dist=False)             # nor dL/dD, dL/dA: the default backward kernels
        d = fused(scene, cam, D, "depth", ups, distortion=False)
        assert runs == [] and len(aux) == 2
        fused(scene, cam, D, "depth", ups)
        assert runs == [1] and len(aux) == 3
    finally:
        _C.DistortionBackward.run, _C.aux_backward_args = orig_run, orig_aux
    for x, y in ((a, b), (c, d)):
        for n in NAMES:
            assert torch.equal(x["grads"][n], y["grads"][n]), n


def test_variant_leaf_parameters():
    """rasterize_leaf_gaussians(distortion=True) against GaussianRasterizer(distortion=True) on the activated tensors: the same map bit
    for bit, the leaves' gradients within check_grads' bars (the band: the packed side's own split composition)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from fused_params import rasterize_leaf_gaussians
    from test_depth_alpha_gpu import LEAF_NAMES, _leaf_params
    scene, cam, D = _scene("B")
    dpix, g, _, _ = _ups(cam.image_height, cam.image_width)
    lp = _leaf_params(scene)
    st = util.hip_settings(scene, cam, D, DEV)

    def leaves():
        t = {k: v.to(DEV).clone().requires_grad_(True) for k, v in lp.items()}
        t["means2D"] = torch.zeros(scene.means3D.shape, device=DEV, requires_grad=True)
        return t

    def packed(u, split):
        act = dict(means3D=u["xyz"], means2D=u["means2D"], opacities=torch.sigmoid(u["opacity"]), scales=torch.exp(u["scaling"]),
                   rotations=torch.nn.functional.normalize(u["rotation"]))
        shs = torch.cat([u["features_dc"], u["features_rest"]], 1)
        out = GaussianRasterizer(st, depth_alpha="depth", distortion=True)(shs=shs, **act)
        if split:
            part = torch.randn(dpix.shape, generator=torch.Generator().manual_seed(99)).to(DEV)
            loss = (out[0] * part).sum() + (GaussianRasterizer(st)(shs=shs, **act)[0] * (dpix - part)).sum()
        else:
            loss = (out[0] * dpix).sum()
        (loss + (out[4] * g).sum()).backward()
        torch.cuda.synchronize()
        return out

    t = leaves()
    out = rasterize_leaf_gaussians(t["xyz"], t["means2D"], t["features_dc"], t["features_rest"], t["opacity"], t["scaling"], t["rotation"],
                                   st, depth_alpha="depth", distortion=True)
    assert len(out) == 5
    ((out[0] * dpix).sum() + (out[4] * g).sum()).backward()
    torch.cuda.synchronize()
    u, w = leaves(), leaves()
    ref = packed(u, False)
    packed(w, True)
    for k in (0, 1, 2, 3, 4):
        assert torch.equal(out[k].detach(), ref[k].detach()), k
    assert float(out[4].detach().max()) > 0
    check_grads(_grads(t, LEAF_NAMES), _grads(u, LEAF_NAMES), [_grads(w, LEAF_NAMES)], "distortion B/leaf", LEAF_NAMES)


# ---- 6. heavy tile -----------------------------------------------------------------------------------------------------------------------
def test_heavy_tile_band_splits_and_depth_segments():
    from diff_gaussian_rasterization import _C
    scene, cam, D = _scene("heavy")
    W, H, P = cam.image_width, cam.image_height, scene.means3D.shape[0]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    ups = _ups(H, W)
    # both splits happen on this path: band entries in the forward's dispatch list, depth segments in the backward's
    R, color, radii, geom, binning, img, depth, alpha, auxbuf = _direct(scene, cam, D, "depth")
    il = _C.image_layout(W, H)

    def entries(count):
        v = img[il.tile_order:il.tile_order + 4 * count].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        return v[v != 0xFFFFFFFF]
    assert int(((entries(T + 3 * min(2048, T // 4)) >> 28) > 0).sum()) >= 4, "no tile was split into bands"
    rng = img[il.ranges:il.ranges + 8 * T].view(torch.int32).view(T, 2)
    assert int((rng[:, 1] - rng[:, 0]).max()) >= 2 * 512, "no list of two checkpoint strides"
    dist, state = _C.distortion_forward(geom, binning, img, R, P, W, H)
    st = util.hip_settings(scene, cam, D, DEV)
    e = torch.empty(0, device=DEV)
    t = {k: getattr(scene, k).to(DEV) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    direct = _C.rasterize_gaussians_backward_depth_alpha("depth", st.bg, t["means3D"], radii, e, t["scales"], t["rotations"], 1.0, e,
                                                         st.viewmatrix, st.projmatrix, st.tanfovx, st.tanfovy, ups[0], t["shs"], D, st.campos,
                                                         geom, R, binning, img, auxbuf, None, None, False,
                                                         distortion=_C.DistortionBackward(state, ups[1]))
    torch.cuda.synchronize()
    assert int(((entries(T + min(4096, T // 2)) >> 28) > 0).sum()) >= 1, "no tile was cut into depth segments"
    f = fused(scene, cam, D, "depth", ups)
    assert torch.equal(f["dist"], dist) and torch.equal(f["grads"]["means3D"], direct[3]) and torch.equal(f["grads"]["opacities"], direct[2])
    r = composition(scene, cam, D, "depth", ups)
    assert torch.equal(f["color"], r["color"])
    d = float((f["dist"] - r["dist"]).abs().max())
    print(f"distortion heavy: map vs the fp32 moment composition {d:.3e} (max {float(f['dist'].max()):.3e})")
    band = composition(scene, cam, D, "depth", ups, split=True)["grads"]
    check_grads(f["grads"], r["grads"], [band], "distortion heavy", NAMES)


# ---- 7. determinism and switches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_determinism_and_debug_switches(name):
    from diff_gaussian_rasterization import _C
    scene, cam, D = _scene(name)
    ups = _ups(cam.image_height, cam.image_width)
    for mode in MODES:
        a = fused(scene, cam, D, mode, ups, use_maps=True)
        runs = [("second run", False), ("GSR_DEBUG_NO_CULL", _C.DEBUG_NO_CULL), ("GSR_DEBUG_NO_TRIM", _C.DEBUG_NO_TRIM)]
        if name == "A":
            runs.append(("GSR_DEBUG_NO_SPLIT", _C.DEBUG_NO_SPLIT))
        for label, debug in runs:
            b = fused(scene, cam, D, mode, ups, use_maps=True, debug=debug)
            for k in ("color", "radii", "depth", "alpha", "dist"):
                assert torch.equal(a[k], b[k]), (name, mode, label, k)
            for n in NAMES:
                assert torch.equal(a["grads"][n], b["grads"][n]), (name, mode, label, n)


# ---- 8. edges ------------------------------------------------------------------------------------------------------------------------------
def _edge_case(label, scene, cam, D, mode):
    """map against the float64 pairwise sum of the device's weights, gradients against the composition"""
    dist, pair, _ = device_maps(scene, cam, D, mode)
    e32 = restatement(label, scene, cam, D, mode)[3]
    err = float((dist.double() - pair).abs().max())
    print(f"distortion {label}/{mode}: device vs pairwise {err:.3e}, fp32 restatement {e32:.3e}, max Dist {float(pair.max()):.3e}")
    assert float(pair.max()) > 0 and err <= 10 * e32, (label, err, e32)
    ups = _ups(cam.image_height, cam.image_width)
    f = fused(scene, cam, D, mode, ups)
    assert torch.equal(f["dist"][0], dist)
    r = composition(scene, cam, D, mode, ups)
    check_grads(f["grads"], r["grads"], [composition(scene, cam, D, mode, ups, split=True)["grads"]], f"distortion {label}/{mode}", NAMES)


def test_edges_empty_culled_and_single():
    cam, D = gsr_scene.make_camera(40, 30), 0
    ups = _ups(30, 40)
    # P = 0
    r = fused(gsr_scene.make_scene(0, -3.0, sh_degree=0, seed=1), cam, D, "depth", ups)
    assert r["dist"].shape == (1, 30, 40) and float(r["dist"].abs().max()) == 0 and r["grads"]["means3D"].shape == (0, 3)
    # a scene behind the camera: nothing is rendered, the map and its gradients are zeros
    scene = gsr_scene.make_scene(500, -3.0, sh_degree=0, seed=2)
    scene = scene._replace(means3D=(scene.means3D * 0.01 - torch.tensor([0.0, 0.0, 20.0])).contiguous())
    for mode in MODES:
        r = fused(scene, cam, D, mode, ups, use_color=False)
        assert int(r["radii"].abs().max()) == 0 and float(r["dist"].abs().max()) == 0
        assert all(float(r["grads"][n].abs().max()) == 0 for n in NAMES)
    # one Gaussian: no pair, Dist is exactly 0 and nothing comes back from it
    scene = gsr_scene.make_scene(1, -1.0, sh_degree=0, seed=3)
    scene = scene._replace(means3D=torch.zeros(1, 3), opacities=torch.full((1, 1), 0.7))
    for mode in MODES:
        r = fused(scene, cam, D, mode, ups, use_color=False)
        assert int(r["radii"].max()) > 0 and float(r["alpha"].max()) > 0.5 and float(r["dist"].abs().max()) == 0
        assert all(float(r["grads"][n].abs().max()) == 0 for n in NAMES)
        with_color = fused(scene, cam, D, mode, ups)
        without = fused(scene, cam, D, mode, ups, use_dist=False, use_maps=False, distortion=False)
        z = fused(scene, cam, D, mode, (ups[0], ups[1], 0 * ups[2], 0 * ups[3]), use_maps=True, distortion=False)   # the aux kernels, zero map gradients
        for n in NAMES:
            assert torch.equal(with_color["grads"][n], z["grads"][n]), (mode, n)
            assert _nerr(with_color["grads"][n], without["grads"][n]) <= 1e-5, (mode, n)
    # under no_grad the map is returned and nothing is saved
    from diff_gaussian_rasterization import GaussianRasterizer
    with torch.no_grad():
        out = GaussianRasterizer(util.hip_settings(scene, cam, D, DEV), depth_alpha="depth", distortion=True)(**_leaves(scene))
    assert len(out) == 5 and all(o.grad_fn is None and not o.requires_grad for o in out)


@pytest.mark.parametrize("size", [(40, 30), (7, 5)])
def test_edges_odd_image_sizes(size):
    W, H = size
    scene, cam, D = gsr_scene.make_scene(300, -2.5, sh_degree=1, seed=14), gsr_scene.make_camera(W, H), 1
    for mode in MODES:
        _edge_case(f"{W}x{H}", scene, cam, D, mode)


def test_edges_invdepth_just_beyond_the_near_plane():
    """view depths from 0.21 on (the near plane culls at 0.2): v = 1 / z up to 4.7, steep in z"""
    scene = gsr_scene.make_scene(300, -5.5, sh_degree=1, seed=15)
    g = torch.Generator().manual_seed(16)
    means = torch.cat([(torch.rand(300, 2, generator=g) - 0.5) * 0.25, -4.0 + 0.21 + 0.5 * torch.rand(300, 1, generator=g)], 1)
    scene = scene._replace(means3D=means.contiguous())
    cam = gsr_scene.make_camera(40, 30)
    o = restatement("near", scene, cam, 1, "invdepth")[0]
    assert 0.2 < float(o["depths"][o["radii"] > 0].min()) < 0.25 and int((o["radii"] > 0).sum()) >= 100
    _edge_case("near", scene, cam, 1, "invdepth")


# ---- 9. render() ---------------------------------------------------------------------------------------------------------------------------
def test_render_adds_distortion_on_both_paths():
    """render(..., depth_alpha=, distortion=True) puts the map into the dict on the activated path and on the leaf path
    (pipe.fused_activations): the first has the bits of GaussianRasterizer(distortion=True) on the model's activated tensors, the
    second agrees with it the way test_renderer_gpu.py's alternates agree (a rounding of an activation may flip a threshold)."""
    import gsr_model
    from diff_gaussian_rasterization import GaussianRasterizer
    from gaussian_renderer import render
    scene, cam, D = _scene("B")
    P = scene.means3D.shape[0]
    camd = cam._replace(world_view_transform=cam.world_view_transform.to(DEV), full_proj_transform=cam.full_proj_transform.to(DEV),
                        camera_center=cam.camera_center.to(DEV))
    g = _ups(cam.image_height, cam.image_width)[1]
    for kw in ({}, dict(fused_activations=True)):
        pc = gsr_model.GaussianParams.from_activated(scene.means3D, scene.shs, scene.scales, scene.rotations, scene.opacities, device=DEV,
                                                     max_sh_degree=D, active_sh_degree=D)
        with torch.no_grad():
            ref = GaussianRasterizer(util.hip_settings(scene, cam, D, DEV), depth_alpha="depth", distortion=True)(
                means3D=pc.get_xyz, means2D=torch.zeros(P, 3, device=DEV), opacities=pc.get_opacity, shs=pc.get_features,
                scales=pc.get_scaling, rotations=pc.get_rotation)
        r = render(camd, pc, gsr_model.pipeline_params(**kw), scene.bg.to(DEV), depth_alpha="depth", distortion=True)
        assert set(r) == {"render", "viewspace_points", "visibility_filter", "radii", "depth", "alpha", "distortion"}
        assert r["distortion"].shape == (1, cam.image_height, cam.image_width)
        if not kw:
            assert torch.equal(r["distortion"].detach(), ref[4]) and torch.equal(r["render"].detach(), ref[0])
        else:
            d = (r["distortion"].detach() - ref[4]).abs()
            assert float(d.mean()) < 1e-6 * max(1.0, float(ref[4].max())) and float((d > 1e-4).float().mean()) < 1e-3, float(d.max())
        (r["distortion"] * g).sum().backward()
        assert float(r["viewspace_points"].grad.abs().max()) > 0 and float(pc._xyz.grad.abs().max()) > 0
        assert "distortion" not in render(camd, pc, gsr_model.pipeline_params(**kw), scene.bg.to(DEV), depth_alpha="depth")
        with pytest.raises(ValueError, match="depth_alpha"):
            render(camd, pc, gsr_model.pipeline_params(**kw), scene.bg.to(DEV), distortion=True)
