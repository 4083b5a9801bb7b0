"""GPU: the median-depth map and the per-pixel Gaussian index maps (GaussianRasterizer(depth_alpha=..., median_depth=True,
index_maps=(median_index, dominant_index, dominant_weight)), rasterize_leaf_gaussians, render(), include/gsr_median.h,
csrc/median.hip).

References.  (1) The definition is checked on weights the device itself produced: one-hot `features=` channels over a tile's list
give every w_i(p) of that tile with the forward's bits, point_list and ranges give the list order, so the dominant weight and
index are compared exactly, with no pixel excluded, and the median is held to its defining property with a margin of 1e-5 on T
(fp32 prefix products of the forward against float64 prefix sums of up to ~1000 weights).  (2) A float64 dense restatement
(tests/torch_splat_median.py) pins the indices independently on a small scene, pixels it calls ambiguous excluded.  (3) Gradients:
float64 autograd through the restatement's gather (tests/test_autograd_cpu.py's bars), and the closed form
dL/dmeans3D_i = (sum_{p : median(p) = i} g(p)) dv_i/dmeans3D_i evaluated in float64 from the device's own index map.  Its bar on the
small scene is 10 x the distance of the fp32 restatement from its float64 self; at size it is 1e-5 of the largest element, the bar
the feature and distortion tests use for tensors without the scale / quaternion chain: the device adds at most a few hundred fp32
terms per Gaussian (2^-24 relative each) and multiplies by one view-matrix column."""
import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
import gsr_scene
import util
from test_distortion_gpu import AUTOGRAD_BARS, _device_v, _direct
from test_features_gpu import NAMES, _cam_settings, _grads, _leaves, _nerr, _scene

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ("depth", "invdepth")
_cache = {}


def _ups(H, W, seed=53):
    """upstream gradients: dL/dpix (3,H,W), dL/dmedian_depth (1,H,W), dL/dD (1,H,W), dL/dA (1,H,W), dL/dDist (1,H,W)"""
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(c, H, W, generator=g).to(DEV) for c in (3, 1, 1, 1, 1))


def _index_maps(H, W, shape3=False):
    """three tensors for index_maps=, pre-filled with values the kernel never writes"""
    s = (1, H, W) if shape3 else (H, W)
    return (torch.full(s, -7, dtype=torch.int32, device=DEV), torch.full(s, -7, dtype=torch.int32, device=DEV),
            torch.full(s, -7.0, dtype=torch.float32, device=DEV))


def fused(scene, cam, D, mode, ups, *, debug=False, use_color=True, use_med=True, use_maps=False, use_dist=True, antialiasing=False,
          camera_grads=False, absgrad=None, densify_stats=None, features=None, dfeat=None, distortion=False, median_depth=True,
          index_maps=True, backward=True):
    """One GaussianRasterizer call -> dict(color, radii, [depth, alpha], [dist], [med], [fmap], [mi, di, dw], grads [incl. "features",
    "V", "PM", "campos"])."""
    from diff_gaussian_rasterization import GaussianRasterizer
    st, cams = _cam_settings(util.hip_settings(scene, cam, D, DEV, debug=debug), camera_grads)
    H, W = cam.image_height, cam.image_width
    t = _leaves(scene)
    kw = dict(camera_grads=True) if camera_grads else {}
    if distortion:
        kw["distortion"] = True
    if median_depth:
        kw["median_depth"] = True
    im = _index_maps(H, W) if index_maps else None
    if im is not None:
        kw["index_maps"] = im
    f = None if features is None else features.to(DEV).clone().requires_grad_(True)
    fk = {} if f is None else dict(features=f)
    out = GaussianRasterizer(st, antialiasing=antialiasing, depth_alpha=mode, absgrad=absgrad, densify_stats=densify_stats, **kw)(**t, **fk)
    n_aux = 0 if mode is None else 2
    assert len(out) == 2 + n_aux + (1 if distortion else 0) + (1 if median_depth else 0) + (0 if f is None else 1)
    r = dict(color=out[0].detach(), radii=out[1])
    if mode is not None:
        r["depth"], r["alpha"] = out[2].detach(), out[3].detach()
    k = 2 + n_aux
    if distortion:
        assert out[k].shape == (1, H, W)
        r["dist"], k = out[k].detach(), k + 1
    if median_depth:
        assert out[k].shape == (1, H, W) and out[k].dtype == torch.float32
        r["med"], med, k = out[k].detach(), out[k], k + 1
    if f is not None:
        assert out[-1].shape == (features.shape[1], H, W) and k == len(out) - 1
        r["fmap"] = out[-1].detach()
    if im is not None:
        r["mi"], r["di"], r["dw"] = im
    if backward:
        dpix, g, dD, dA, gdist = ups
        loss = 0
        if use_color:
            loss = loss + (out[0] * dpix).sum()
        if use_med and median_depth:
            loss = loss + (med * g).sum()
        if use_maps:
            loss = loss + (out[2] * dD).sum() + (out[3] * dA).sum()
        if use_dist and distortion:
            loss = loss + (out[4] * gdist).sum()
        if f is not None and dfeat is not None:
            loss = loss + (out[-1] * dfeat).sum()
        loss.backward()
        torch.cuda.synchronize()
        r["grads"] = _grads(t, NAMES)
        if f is not None:
            r["grads"]["features"] = None if f.grad is None else f.grad.clone()
        for n, c in zip(("V", "PM", "campos"), cams):
            r["grads"][n] = c.grad.clone() if c.grad is not None else torch.zeros_like(c)
    return r


def direct(scene, cam, D, mode, debug=0, antialiasing=False, median_debug=None):
    """_C.rasterize_gaussians_depth_alpha and _C.median_forward on its state -> dict(med (1,H,W), state, mi, di, dw, + the forward's
    R, radii, geom, binning, img, aux, color, depth, alpha)"""
    from diff_gaussian_rasterization import _C
    P, W, H = scene.means3D.shape[0], cam.image_width, cam.image_height
    R, color, radii, geom, binning, img, depth, alpha, aux = _direct(scene, cam, D, mode, debug=debug, antialiasing=antialiasing)
    im = _index_maps(H, W)
    med, state = _C.median_forward(geom, binning, img, R, P, W, H, index_maps=im, debug=debug if median_debug is None else median_debug)
    torch.cuda.synchronize()
    return dict(R=R, color=color, radii=radii, geom=geom, binning=binning, img=img, depth=depth, alpha=alpha, aux=aux, med=med, state=state,
                mi=im[0], di=im[1], dw=im[2])


def closed_form(scene, cam, mode, median_index, g):
    """-> float64 (dL/dmeans3D (P, 3), G (P,), hom (P, 4)) of the loss sum(median_depth * g) from an index map: G_i = the sum of g over
    the pixels whose median is i, v_i = z_i = hom_i . V[:, 2] or its reciprocal"""
    P = scene.means3D.shape[0]
    idx, gg = median_index.reshape(-1).long().cpu(), g.reshape(-1).double().cpu()
    hit = idx >= 0
    G = torch.zeros(P, dtype=torch.float64).index_add_(0, idx[hit], gg[hit])
    V = cam.world_view_transform.double()
    hom = torch.cat([scene.means3D.double(), torch.ones(P, 1, dtype=torch.float64)], 1)
    z = hom @ V[:, 2]
    dv = torch.ones(P, dtype=torch.float64) if mode == "depth" else -1.0 / (z * z)
    return (G * dv)[:, None] * V[:3, 2][None], G * dv, hom


def check_closed_form(label, grads, scene, cam, mode, median_index, g, bar=1e-5, others_zero=True):
    ref, _, _ = closed_form(scene, cam, mode, median_index, g)
    e = _nerr(grads["means3D"].cpu(), ref)
    line = f"median {label} dL/dmeans3D vs the closed form of the device's index map: err {e:.2e} bar {bar:.2e}"
    print(line)
    util.parity_log(line)
    assert float(ref.abs().max()) > 0 and e <= bar, (label, e, bar)
    if others_zero:   # the median depth is differentiable in v only
        for n in NAMES:
            if n != "means3D":
                assert float(grads[n].abs().max()) == 0.0, (label, n)


def check_definition(label, r, scene, cam, tiles=None):
    """The definition on the device's own weights, for every pixel of the tiles given (default: all) -> (pixels whose median is their
    last hit, pixels whose median is not).  r: the dict of direct()."""
    from diff_gaussian_rasterization import _C
    P, W, H = scene.means3D.shape[0], cam.image_width, cam.image_height
    gx, gy = (W + 15) // 16, (H + 15) // 16
    R = int(r["R"])
    il = _C.image_layout(W, H)
    ncontrib = r["img"][il.n_contrib:il.n_contrib + 4 * W * H].view(torch.int32).view(H, W)
    med, state, mi, di, dw = r["med"][0], r["state"], r["mi"], r["di"], r["dw"]
    hit = ncontrib > 0
    # indices are -1 and values 0 exactly where nothing blended
    assert torch.equal(mi >= 0, hit) and torch.equal(di >= 0, hit) and torch.equal(state >= 0, hit)
    assert bool((mi[~hit] == -1).all()) and bool((di[~hit] == -1).all()) and bool((state[~hit] == -1).all())
    assert bool((dw[~hit] == 0).all()) and bool((med[~hit] == 0).all()) and bool((dw[hit] > 0).all())
    assert int(mi.max()) < P and int(di.max()) < P
    # the depth is the record's, bit for bit
    v = _device_v(r["geom"], r["radii"])
    assert torch.equal(med, torch.where(hit, v[mi.clamp_min(0).long()], torch.zeros_like(med)))
    if R == 0:
        assert not bool(hit.any())
        return 0, 0
    rng = r["img"][il.ranges:il.ranges + 8 * gx * gy].view(torch.int32).view(gx * gy, 2).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    bl = _C.binning_layout(P, R, W, H)
    plist = r["binning"][bl.point_list:bl.point_list + 4 * R].view(torch.int32)
    n_last = n_before = 0
    for t in (range(gx * gy) if tiles is None else tiles):
        r0, r1 = int(rng[t, 0]), int(rng[t, 1])
        ys, xs = slice(16 * (t // gx), min(H, 16 * (t // gx) + 16)), slice(16 * (t % gx), min(W, 16 * (t % gx) + 16))
        if r1 <= r0:
            assert not bool(hit[ys, xs].any()), (label, t)
            continue
        ids = plist[r0:r1].long()
        n = ids.numel()
        assert int(ids.unique().numel()) == n   # a tile's list holds a Gaussian once: distinct positions are distinct gradient slots
        w = []
        for c0 in range(0, n, 1024):   # one-hot channels over this tile's list: w_i(p) with the forward's bits
            c1 = min(n, c0 + 1024)
            onehot = torch.zeros(P, c1 - c0, device=DEV)
            onehot[ids[c0:c1], torch.arange(c1 - c0, device=DEV)] = 1.0
            w.append(_C.features_forward(r["geom"], r["binning"], r["img"], R, P, W, H, onehot)[:, ys, xs].reshape(c1 - c0, -1))
        w = torch.cat(w, 0)
        pos = torch.arange(n, device=DEV)[:, None]
        blended = w > 0
        h = hit[ys, xs].reshape(-1)
        assert torch.equal(blended.any(0), h), (label, t)
        # dominant: the columnwise maximum, exactly, and its first position in list order
        top = w.max(0).values
        assert torch.equal(dw[ys, xs].reshape(-1), top), (label, t)
        first = torch.where(w == top[None], pos, n).min(0).values
        assert torch.equal(di[ys, xs].reshape(-1)[h].long(), ids[first[h]]), (label, t)
        # median: a blended Gaussian with T > 0.5 in front of it, and behind it T <= 0.5 unless it is the last blended one
        inv = torch.full((P,), -1, dtype=torch.int64, device=DEV)
        inv[ids] = torch.arange(n, device=DEV)
        m = inv[mi[ys, xs].reshape(-1).clamp_min(0).long()]
        assert bool((m[h] >= 0).all()), (label, t, "a median that is not in the tile's list")
        assert torch.equal(state[ys, xs].reshape(-1)[h].long(), m[h]), (label, t, "the state is not the median's list position")
        m = m.clamp_min(0)
        w64 = w.double()
        cum = w64.cumsum(0)
        t_in, t_out = (1.0 - (cum - w64)).gather(0, m[None])[0], (1.0 - cum).gather(0, m[None])[0]
        assert bool(blended.gather(0, m[None])[0][h].all()), (label, t, "a median that did not blend")
        assert bool((t_in[h] > 0.5 - 1e-5).all()), (label, t, float(t_in[h].min()))
        is_last = m == torch.where(blended, pos, -1).max(0).values
        assert bool((is_last | (t_out <= 0.5 + 1e-5))[h].all()), (label, t, float(t_out[h & ~is_last].max()))
        n_last += int((is_last & h).sum())
        n_before += int((~is_last & h).sum())
    return n_last, n_before


# ---- 1. the definition, on the device's own weights, no pixel excluded ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("mode", MODES)
def test_definition_on_the_devices_own_weights(name, mode):
    from test_features_gpu import _ranges
    scene, cam, D = _scene(name)
    if name == "A":
        rng = _ranges(scene, cam, D)
        assert int((rng[:, 1] - rng[:, 0]).max()) >= 1024, "scene A no longer has a heavy tile"
        assert cam.image_width % 16 == 1 and cam.image_height % 16 == 1   # a one-pixel tile column and row
    r = direct(scene, cam, D, mode)
    n_last, n_before = check_definition(f"{name}/{mode}", r, scene, cam)
    print(f"median {name}/{mode}: {n_last} pixels whose median is their last hit, {n_before} whose transmittance crossed 0.5")
    assert n_last > 0 and n_before > 0, "both branches of the median must occur on this scene"


# ---- 2. against the float64 restatement ------------------------------------------------------------------------------------------------------
def _small_reference(mode):
    """-> dict: scene, cam, maps (the float64 restatement's), ok, dpix, g, ref (float64 gradients of the combined loss), ref_med (of
    sum(median_depth g) alone), d32 (the fp32 restatement's distance from it, dL/dmeans3D); the reference-side checks run here, with
    no device"""
    if ("small", mode) not in _cache:
        import torch_splat_median as tm
        from test_features_gpu import SMALL, _small
        scene, cam, o = _small()
        s = SMALL
        gen = torch.Generator().manual_seed(6)
        dpix, g = torch.randn(3, s["H"], s["W"], generator=gen), torch.randn(1, s["H"], s["W"], generator=gen)
        res = {}
        for dt in (torch.float64, torch.float32):
            leaf = lambda x: x.to(dt).clone().requires_grad_(True)
            t = dict(means3D=leaf(scene.means3D), scales=leaf(scene.scales), rotations=leaf(scene.rotations), opacities=leaf(scene.opacities),
                     shs=leaf(scene.shs))
            img, _, _, med, maps = tm.render(o, t["means3D"], t["scales"], t["rotations"], t["opacities"], t["shs"], mode, dtype=dt)
            if dt == torch.float64:
                ok = ~maps["ambiguous"]
                share = float((~ok).float().mean())
                hit, crossed = maps["hit"], maps["crossed"]
                print(f"median small scene: excluded share {share:.4f}; hit {float(hit.float().mean()):.3f}; crossed 0.5: "
                      f"{float(crossed.float().sum() / hit.float().sum()):.3f} of those; {int(maps['median_index'][hit].unique().numel())} medians")
                assert share <= 0.05, share
                assert bool(crossed.any()) and bool((hit & ~crossed).any())
                dpix, g = dpix * ok, g * ok
                keep = maps
            else:   # outside the excluded pixels an fp32 evaluation makes the same choices
                assert torch.equal(maps["median_index"][ok], keep["median_index"][ok])
                assert torch.equal(maps["dominant_index"][ok], keep["dominant_index"][ok])
            gm = torch.autograd.grad((med * g[0].to(dt)).sum(), list(t.values()), retain_graph=True, allow_unused=True)
            ((img * dpix.to(dt)).sum() + (med * g[0].to(dt)).sum()).backward()
            res[dt] = ({n: v.grad.double() for n, v in t.items()},
                       {n: (torch.zeros_like(v).double() if x is None else x.double()) for (n, v), x in zip(t.items(), gm)})
        for n, bar in AUTOGRAD_BARS.items():   # the bars can be asked of an fp32 evaluation on this scene
            e = _nerr(res[torch.float32][0][n], res[torch.float64][0][n])
            print(f"median small scene/{mode}, fp32 restatement dL/d{n}: err {e:.2e} bar {bar:.2e}")
            assert e <= 0.5 * bar, (n, e, bar)
        d32 = _nerr(res[torch.float32][1]["means3D"], res[torch.float64][1]["means3D"])
        assert 0 < d32 < 1e-5, d32
        for n in ("scales", "rotations", "opacities", "shs"):   # the gather has no other argument
            assert float(res[torch.float64][1][n].abs().max()) == 0.0, n
        _cache[("small", mode)] = dict(scene=scene, cam=cam, maps=keep, ok=ok, dpix=dpix, g=g, ref=res[torch.float64][0],
                                       ref_med=res[torch.float64][1], d32=d32)
    return _cache[("small", mode)]


@pytest.mark.parametrize("mode", MODES)
def test_indices_match_the_float64_restatement(mode):
    from test_features_gpu import SMALL
    s = _small_reference(mode)
    r = direct(s["scene"], s["cam"], SMALL["D"], mode)
    ok = s["ok"]
    for k, n in (("mi", "median_index"), ("di", "dominant_index")):
        same = r[k].cpu().long() == s["maps"][n]
        print(f"median small scene/{mode}: {n} differs on {int((~same).sum())} pixels, {int((~same & ok).sum())} of them not excluded")
        assert bool(same[ok].all()), n
    assert torch.equal((r["mi"].cpu() >= 0)[ok], s["maps"]["hit"][ok])
    e = float((r["dw"].cpu().double() - s["maps"]["dominant_weight"]).abs()[ok].max())
    print(f"median small scene/{mode}: dominant weight vs float64 {e:.2e}")
    n_last, n_before = check_definition(f"small/{mode}", r, s["scene"], s["cam"])
    assert n_last > 0 and n_before > 0


# ---- 3. gradients --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_gradients_match_float64_autograd(mode):
    from test_features_gpu import SMALL
    s = _small_reference(mode)
    z = torch.zeros(1, SMALL["H"], SMALL["W"], device=DEV)
    f = fused(s["scene"], s["cam"], SMALL["D"], mode, (s["dpix"].to(DEV), s["g"].to(DEV), z, z, z))
    assert bool((f["mi"].cpu().long() == s["maps"]["median_index"])[s["ok"]].all())
    for n, bar in AUTOGRAD_BARS.items():
        e = _nerr(f["grads"][n].cpu().reshape(s["ref"][n].shape), s["ref"][n])
        line = f"median float64 autograd/{mode} dL/d{n}: err {e:.2e} bar {bar:.2e}"
        print(line)
        util.parity_log(line)
        assert e < bar, (n, e, bar)


@pytest.mark.parametrize("mode", MODES)
def test_median_gradient_alone_is_the_closed_form(mode):
    from test_features_gpu import SMALL
    s = _small_reference(mode)
    z = torch.zeros(1, SMALL["H"], SMALL["W"], device=DEV)
    f = fused(s["scene"], s["cam"], SMALL["D"], mode, (s["dpix"].to(DEV), s["g"].to(DEV), z, z, z), use_color=False)
    # the closed form of the restatement's own index map is its autograd result: the helper restates the definition
    own = closed_form(s["scene"], s["cam"], mode, s["maps"]["median_index"], s["g"])[0]
    assert _nerr(own, s["ref_med"]["means3D"]) < 1e-12
    print(f"median small scene/{mode}: fp32 restatement vs float64, dL/dmeans3D of the median loss alone: {s['d32']:.2e}")
    check_closed_form(f"small/{mode}", f["grads"], s["scene"], s["cam"], mode, f["mi"], s["g"], bar=10 * s["d32"])
    assert _nerr(f["grads"]["means3D"].cpu(), s["ref_med"]["means3D"]) <= 10 * s["d32"]


# ---- 4. nothing else moves -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_nothing_else_moves(mode):
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    scene, cam, D = _scene("A")
    P, W, H = scene.means3D.shape[0], cam.image_width, cam.image_height
    R, color, radii, geom, binning, img, depth, alpha, aux = _direct(scene, cam, D, mode)
    before = [b.clone() for b in (geom, binning, img, aux, color, radii, depth, alpha)]
    im = _index_maps(H, W)
    med, state = _C.median_forward(geom, binning, img, R, P, W, H, index_maps=im)
    torch.cuda.synchronize()
    for a, b, n in zip(before, (geom, binning, img, aux, color, radii, depth, alpha),
                       ("geometry", "binning", "image", "aux scratch", "colour", "radii", "depth", "alpha")):
        assert torch.equal(a, b), f"gsr_median_forward wrote the {n}"
    assert med.shape == (1, H, W) and state.shape == (H, W) and state.dtype == torch.int32 and float(med.abs().max()) > 0
    # outputs that were not asked for are not needed: each subset gives the same tensors
    for pick in ((0,), (1,), (2,), (0, 2)):
        sub = _index_maps(H, W)
        part = tuple(t if i in pick else None for i, t in enumerate(sub))
        m2, s2 = _C.median_forward(geom, binning, img, R, P, W, H, index_maps=part, depth=(pick == (1,)))
        for i in pick:
            assert torch.equal(sub[i], im[i]), pick
        assert (m2 is None and s2 is None) if pick != (1,) else (torch.equal(m2, med) and torch.equal(s2, state))
    m2, s2 = _C.median_forward(geom, binning, img, R, P, W, H)
    assert torch.equal(m2, med) and torch.equal(s2, state)
    # the module: every other output with the new keywords is what it is without them, all five features of the family together
    ups = _ups(H, W)
    feats = torch.randn(P, 3, generator=torch.Generator().manual_seed(41))
    a = fused(scene, cam, D, mode, ups, distortion=True, features=feats, backward=False)
    b = fused(scene, cam, D, mode, ups, distortion=True, features=feats, backward=False, median_depth=False, index_maps=False)
    for k in ("color", "radii", "depth", "alpha", "dist", "fmap"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["color"], color) and torch.equal(a["depth"], depth) and torch.equal(a["med"], med)
    for k, t in zip(("mi", "di", "dw"), im):
        assert torch.equal(a[k], t), k
    # a backward without a gradient on the map is the parent's, bit for bit, and runs nothing of this feature
    runs = []
    orig = _C.MedianBackward.run
    _C.MedianBackward.run = lambda self, *x: (runs.append(1), orig(self, *x))[1]
    try:
        for kw in (dict(use_maps=True), dict()):   # with dL/dD and dL/dA: the aux kernels; without: the default ones
            x = fused(scene, cam, D, mode, ups, use_med=False, **kw)
            y = fused(scene, cam, D, mode, ups, median_depth=False, index_maps=False, **kw)
            assert runs == []
            for n in NAMES:
                assert torch.equal(x["grads"][n], y["grads"][n]), n
        fused(scene, cam, D, mode, ups)
        assert runs == [1]
    finally:
        _C.MedianBackward.run = orig
    # the default call's outputs are what they were
    c, rr = GaussianRasterizer(util.hip_settings(scene, cam, D, DEV))(**_leaves(scene))
    assert torch.equal(c.detach(), color) and torch.equal(rr, radii)
    # index_maps alone: without depth_alpha, under no_grad, in (1, H, W) tensors; the tuple is unchanged
    im1 = _index_maps(H, W, shape3=True)
    with torch.no_grad():
        out = GaussianRasterizer(util.hip_settings(scene, cam, D, DEV), index_maps=im1)(**_leaves(scene))
    torch.cuda.synchronize()
    assert len(out) == 2 and torch.equal(out[0], color) and all(o.grad_fn is None for o in out)
    for t, ref in zip(im1, im):
        assert torch.equal(t[0], ref)
    # ... and with gradients enabled the backward is the default one
    im2 = _index_maps(H, W)
    t = _leaves(scene)
    out = GaussianRasterizer(util.hip_settings(scene, cam, D, DEV), index_maps=(None, im2[1], None))(**t)
    assert len(out) == 2
    (out[0] * ups[0]).sum().backward()
    u = _leaves(scene)
    (GaussianRasterizer(util.hip_settings(scene, cam, D, DEV))(**u)[0] * ups[0]).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(im2[1], im[1]) and bool((im2[0] == -7).all()) and bool((im2[2] == -7).all())
    for n in NAMES:
        assert torch.equal(t[n].grad, u[n].grad), n


def test_without_an_aux_mode_the_depth_is_zero_and_the_indices_are_valid():
    from diff_gaussian_rasterization import _C
    from test_features_gpu import _state
    scene, cam, D = _scene("A")
    P, W, H = scene.means3D.shape[0], cam.image_width, cam.image_height
    R, color, radii, geom, binning, img = _state(scene, cam, D)
    im = _index_maps(H, W)
    med, state = _C.median_forward(geom, binning, img, R, P, W, H, index_maps=im)
    ref = direct(scene, cam, D, "depth")
    assert float(med.abs().max()) == 0.0 and torch.equal(state, ref["state"])
    for t, k in zip(im, ("mi", "di", "dw")):
        assert torch.equal(t, ref[k]), k


# ---- 5. variants on B ------------------------------------------------------------------------------------------------------------------------
def test_variant_antialiasing():
    scene, cam, D = _scene("B")
    r = direct(scene, cam, D, "depth", antialiasing=True)
    n_last, n_before = check_definition("B/antialiasing", r, scene, cam)
    assert n_last > 0 and n_before > 0
    plain = direct(scene, cam, D, "depth")
    assert not torch.equal(r["dw"], plain["dw"]) and not torch.equal(r["mi"], plain["mi"])
    ups = _ups(cam.image_height, cam.image_width)
    f = fused(scene, cam, D, "depth", ups, antialiasing=True, use_color=False)
    for k in ("med", "mi", "di", "dw"):
        assert torch.equal(f[k].reshape(r[k].shape), r[k]), k
    check_closed_form("B/antialiasing", f["grads"], scene, cam, "depth", f["mi"], ups[1])


@pytest.mark.parametrize("mode", MODES)
def test_variant_camera_grads(mode):
    """The median loss alone with camera_grads: v_i = hom_i . V[:, 2], so dL/dV[k][2] = sum_i (G dv)_i hom_ik and nothing else of the
    three camera tensors gets a gradient.  The bar is test_camera_grads_gpu.py's, as the distortion test takes it: 1e-5 of the largest
    sum over the Gaussians of the terms' moduli.  The Gaussians' gradients with the camera kernels are the closed form too."""
    scene, cam, D = _scene("B")
    ups = _ups(cam.image_height, cam.image_width)
    f = fused(scene, cam, D, mode, ups, camera_grads=True, use_color=False)
    check_closed_form(f"B/{mode}/camera_grads", f["grads"], scene, cam, mode, f["mi"], ups[1])
    _, Gdv, hom = closed_form(scene, cam, mode, f["mi"], ups[1])
    ref = torch.zeros(4, 4, dtype=torch.float64)
    ref[:, 2] = (Gdv[:, None] * hom).sum(0)
    bar = 1e-5 * float((Gdv[:, None] * hom).abs().sum(0).max())
    e = float((f["grads"]["V"].cpu().double() - ref).abs().max())
    line = f"median B/{mode}/camera_grads dL/dV: err {e:.3e} bar {bar:.3e}"
    print(line)
    util.parity_log(line)
    assert float(ref.abs().max()) > 0 and e <= bar, (e, bar)
    assert float(f["grads"]["PM"].abs().max()) == 0.0 and float(f["grads"]["campos"].abs().max()) == 0.0
    # with the colour in the loss, the camera gradient is the colour's plus this one
    both = fused(scene, cam, D, mode, ups, camera_grads=True)
    zero_maps = (ups[0], ups[1], 0 * ups[2], 0 * ups[3], ups[4])
    col = fused(scene, cam, D, mode, zero_maps, camera_grads=True, use_med=False, use_maps=True)   # the aux kernels, zero map gradients
    for n in ("PM", "campos"):
        assert torch.equal(both["grads"][n], col["grads"][n]), n
    e = float(((both["grads"]["V"] - col["grads"]["V"]).cpu().double() - ref).abs().max())
    bar2 = bar + 1e-5 * float(col["grads"]["V"].abs().max())   # ... rounded once more at the size of the colour's
    print(f"median B/{mode}/camera_grads dL/dV with the colour: err {e:.3e} bar {bar2:.3e}")
    assert e <= bar2, (e, bar2)


def test_variant_distortion_features_and_median_together():
    """(color, radii, depth, alpha, distortion, median_depth, feature_map); the median's gradient reaches means3D alone, so every other
    leaf has the bits of the run without it, and means3D differs by the closed form."""
    scene, cam, D = _scene("B")
    P, K = scene.means3D.shape[0], 4
    H, W = cam.image_height, cam.image_width
    ups = _ups(H, W)
    feats = torch.randn(P, K, generator=torch.Generator().manual_seed(41))
    gf = torch.randn(K, H, W, generator=torch.Generator().manual_seed(43)).to(DEV)
    both = fused(scene, cam, D, "depth", ups, features=feats, dfeat=gf, distortion=True, use_maps=True)    # fused() asserts the order
    other = fused(scene, cam, D, "depth", ups, features=feats, dfeat=gf, distortion=True, use_maps=True, median_depth=False, index_maps=False)
    alone = fused(scene, cam, D, "depth", ups, use_color=False)
    assert torch.equal(both["dist"], other["dist"]) and torch.equal(both["fmap"], other["fmap"]) and torch.equal(both["med"], alone["med"])
    assert both["med"].shape == (1, H, W) and both["dist"].shape == (1, H, W) and both["fmap"].shape == (K, H, W)
    for n in NAMES + ("features",):
        if n != "means3D":
            assert torch.equal(both["grads"][n], other["grads"][n]), n
    ref = closed_form(scene, cam, "depth", both["mi"], ups[1])[0]
    d = (both["grads"]["means3D"] - other["grads"]["means3D"]).cpu().double()
    bar = 1e-5 * float(both["grads"]["means3D"].abs().max())   # the sum is rounded at the size of the total
    e = float((d - ref).abs().max())
    print(f"median B/distortion+features+median dL/dmeans3D share: err {e:.3e} bar {bar:.3e}")
    assert e <= bar and float(ref.abs().max()) > 100 * bar, (e, bar)


def test_variant_densify_stats_and_absgrad_do_not_see_the_median():
    scene, cam, D = _scene("B")
    P = scene.means3D.shape[0]
    ups = _ups(cam.image_height, cam.image_width)
    res = []
    for use_med in (True, False):
        stats = tuple(torch.zeros(P, device=DEV) for _ in range(3))
        ab = (torch.full((P, 2), 7.0, device=DEV), torch.zeros(P, device=DEV))
        f = fused(scene, cam, D, "depth", ups, use_maps=True, use_med=use_med, densify_stats=stats, absgrad=ab)
        res.append((stats, ab, f))
    for a, b in zip(res[0][0] + res[0][1], res[1][0] + res[1][1]):
        assert torch.equal(a, b)
    assert float(res[0][0][0].abs().max()) > 0 and float(res[0][1][0].abs().max()) > 0
    assert torch.equal(res[0][2]["grads"]["means2D"], res[1][2]["grads"]["means2D"])
    assert not torch.equal(res[0][2]["grads"]["means3D"], res[1][2]["grads"]["means3D"])


def test_variant_leaf_parameters():
    """rasterize_leaf_gaussians(median_depth=True, index_maps=) against GaussianRasterizer on the activated tensors: the maps bit for
    bit, and xyz's gradient the closed form."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from fused_params import rasterize_leaf_gaussians
    from test_depth_alpha_gpu import _leaf_params
    scene, cam, D = _scene("B")
    H, W = cam.image_height, cam.image_width
    g = _ups(H, W)[1]
    lp = _leaf_params(scene)
    st = util.hip_settings(scene, cam, D, DEV)
    t = {k: v.to(DEV).clone().requires_grad_(True) for k, v in lp.items()}
    t["means2D"] = torch.zeros(scene.means3D.shape, device=DEV, requires_grad=True)
    im = _index_maps(H, W)
    out = rasterize_leaf_gaussians(t["xyz"], t["means2D"], t["features_dc"], t["features_rest"], t["opacity"], t["scaling"], t["rotation"],
                                   st, depth_alpha="depth", distortion=True, median_depth=True, index_maps=im)
    assert len(out) == 6 and out[5].shape == (1, H, W)
    (out[5] * g).sum().backward()
    torch.cuda.synchronize()
    with torch.no_grad():
        im2 = _index_maps(H, W)
        ref = GaussianRasterizer(st, depth_alpha="depth", distortion=True, median_depth=True, index_maps=im2)(
            means3D=t["xyz"], means2D=t["means2D"], opacities=torch.sigmoid(t["opacity"]), scales=torch.exp(t["scaling"]),
            rotations=torch.nn.functional.normalize(t["rotation"]), shs=torch.cat([t["features_dc"], t["features_rest"]], 1))
    for k in range(6):
        assert torch.equal(out[k].detach(), ref[k]), k
    for a, b in zip(im, im2):
        assert torch.equal(a, b)
    assert float(out[5].detach().abs().max()) > 0
    check_closed_form("B/leaf", dict(means3D=t["xyz"].grad), scene, cam, "depth", im[0], g, others_zero=False)
    for n in ("means2D", "features_dc", "features_rest", "opacity", "scaling", "rotation"):
        assert t[n].grad is None or float(t[n].grad.abs().max()) == 0.0, n


# ---- 6. heavy tile ---------------------------------------------------------------------------------------------------------------------------
def test_heavy_tile_band_splits_and_depth_segments():
    from diff_gaussian_rasterization import _C
    scene, cam, D = _scene("heavy")
    W, H, P = cam.image_width, cam.image_height, scene.means3D.shape[0]
    gx = (W + 15) // 16
    T = gx * ((H + 15) // 16)
    ups = _ups(H, W)
    # both splits happen on this path: band entries in the forward's dispatch list, depth segments in the backward's
    r = direct(scene, cam, D, "depth")
    img = r["img"]
    il = _C.image_layout(W, H)

    def entries(count):
        v = img[il.tile_order:il.tile_order + 4 * count].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        return v[v != 0xFFFFFFFF]
    assert int(((entries(T + 3 * min(2048, T // 4)) >> 28) > 0).sum()) >= 4, "no tile was split into bands"
    rng = img[il.ranges:il.ranges + 8 * T].view(torch.int32).view(T, 2)
    lens = (rng[:, 1] - rng[:, 0]).cpu()
    assert int(lens.max()) >= 2 * 512, "no list of two checkpoint strides"
    # the definition on the heaviest tile and on the lightest one that has a list
    heaviest = int(lens.argmax())
    light = int(torch.where(lens > 0, lens, lens.max()).argmin())
    n_last, n_before = check_definition("heavy", r, scene, cam, tiles=sorted({heaviest, light}))
    print(f"median heavy: tile {heaviest} holds {int(lens.max())} instances; {n_last} medians are the last hit, {n_before} are not")
    assert n_before > 0
    full = direct(scene, cam, D, "depth", median_debug=_C.DEBUG_MEDIAN_FULL_WALK)
    for k in ("med", "state", "mi", "di", "dw"):
        assert torch.equal(r[k], full[k]), k
    st = util.hip_settings(scene, cam, D, DEV)
    e = torch.empty(0, device=DEV)
    t = {k: getattr(scene, k).to(DEV) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    grads = _C.rasterize_gaussians_backward_depth_alpha("depth", st.bg, t["means3D"], r["radii"], e, t["scales"], t["rotations"], 1.0, e,
                                                        st.viewmatrix, st.projmatrix, st.tanfovx, st.tanfovy, ups[0], t["shs"], D, st.campos,
                                                        r["geom"], r["R"], r["binning"], img, r["aux"], None, None, False,
                                                        median=_C.MedianBackward(r["state"], ups[1]))
    torch.cuda.synchronize()
    assert int(((entries(T + min(4096, T // 2)) >> 28) > 0).sum()) >= 1, "no tile was cut into depth segments"
    f = fused(scene, cam, D, "depth", ups)
    for k in ("med", "mi", "di", "dw"):
        assert torch.equal(f[k].reshape(r[k].shape), r[k]), k
    assert torch.equal(f["grads"]["means3D"], grads[3]) and torch.equal(f["grads"]["opacities"], grads[2])
    alone = fused(scene, cam, D, "depth", ups, use_color=False)
    check_closed_form("heavy", alone["grads"], scene, cam, "depth", alone["mi"], ups[1])


# ---- 7. determinism and switches -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_determinism_and_debug_switches(name):
    from diff_gaussian_rasterization import _C
    scene, cam, D = _scene(name)
    ups = _ups(cam.image_height, cam.image_width)
    for mode in MODES:
        a = fused(scene, cam, D, mode, ups, use_maps=True)
        runs = [("second run", False), ("GSR_DEBUG_NO_CULL", _C.DEBUG_NO_CULL), ("GSR_DEBUG_NO_TRIM", _C.DEBUG_NO_TRIM),
                ("GSR_DEBUG_MEDIAN_FULL_WALK", _C.DEBUG_MEDIAN_FULL_WALK)]
        if name == "A":
            runs.append(("GSR_DEBUG_NO_SPLIT", _C.DEBUG_NO_SPLIT))
        for label, debug in runs:
            b = fused(scene, cam, D, mode, ups, use_maps=True, debug=debug)
            for k in ("color", "radii", "depth", "alpha", "med", "mi", "di", "dw"):
                assert torch.equal(a[k], b[k]), (name, mode, label, k)
            for n in NAMES:
                assert torch.equal(a["grads"][n], b["grads"][n]), (name, mode, label, n)
        # the early exit against the full walk, the state included, with and without the culling
        x = direct(scene, cam, D, mode)
        for dbg in (_C.DEBUG_MEDIAN_FULL_WALK, _C.DEBUG_MEDIAN_FULL_WALK | _C.DEBUG_NO_CULL, _C.DEBUG_NO_CULL):
            y = direct(scene, cam, D, mode, median_debug=dbg)
            for k in ("med", "state", "mi", "di", "dw"):
                assert torch.equal(x[k], y[k]), (name, mode, dbg, k)


# ---- 8. edges --------------------------------------------------------------------------------------------------------------------------------
def test_edges_empty_culled_and_single():
    from diff_gaussian_rasterization import _C
    cam, D = gsr_scene.make_camera(40, 30), 0
    ups = _ups(30, 40)
    # P = 0
    r = fused(gsr_scene.make_scene(0, -3.0, sh_degree=0, seed=1), cam, D, "depth", ups)
    assert r["med"].shape == (1, 30, 40) and float(r["med"].abs().max()) == 0 and r["grads"]["means3D"].shape == (0, 3)
    assert bool((r["mi"] == -1).all()) and bool((r["di"] == -1).all()) and bool((r["dw"] == 0).all())
    # a scene behind the camera: nothing is rendered (num_rendered == 0), the outputs are fills and the gradients zeros
    scene = gsr_scene.make_scene(500, -3.0, sh_degree=0, seed=2)
    scene = scene._replace(means3D=(scene.means3D * 0.01 - torch.tensor([0.0, 0.0, 20.0])).contiguous())
    for mode in MODES:
        r = fused(scene, cam, D, mode, ups, use_color=False)
        assert int(r["radii"].abs().max()) == 0 and float(r["med"].abs().max()) == 0
        assert bool((r["mi"] == -1).all()) and bool((r["di"] == -1).all()) and bool((r["dw"] == 0).all())
        assert all(float(r["grads"][n].abs().max()) == 0 for n in NAMES)
        d = direct(scene, cam, D, mode)
        assert d["R"] == 0 and bool((d["state"] == -1).all()) and bool((d["mi"] == -1).all()) and float(d["med"].abs().max()) == 0
    # one Gaussian: it is the median and the dominant of every pixel it blends into
    scene = gsr_scene.make_scene(1, -1.0, sh_degree=0, seed=3)
    scene = scene._replace(means3D=torch.zeros(1, 3), opacities=torch.full((1, 1), 0.7))
    for mode in MODES:
        r = fused(scene, cam, D, mode, ups, use_color=False)
        hit = r["alpha"][0] > 0
        assert int(r["radii"].max()) > 0 and float(r["alpha"].max()) > 0.5
        assert torch.equal(r["mi"], torch.where(hit, 0, -1).int()) and torch.equal(r["di"], r["mi"])
        # one hit: w = alpha, and the alpha map is 1 - (1 - alpha), rounded twice
        assert float((r["dw"] - r["alpha"][0]).abs().max()) <= 2e-7 and bool((r["dw"][~hit] == 0).all())
        z = float(cam.world_view_transform[3, 2])
        v = z if mode == "depth" else 1.0 / z
        assert float((r["med"][0][hit] - v).abs().max()) <= 1e-6 * abs(v) and bool((r["med"][0][~hit] == 0).all())
        check_closed_form(f"single/{mode}", r["grads"], scene, cam, mode, r["mi"], ups[1])
    # under no_grad the map is returned and nothing is saved
    from diff_gaussian_rasterization import GaussianRasterizer
    with torch.no_grad():
        out = GaussianRasterizer(util.hip_settings(scene, cam, D, DEV), depth_alpha="depth", median_depth=True)(**_leaves(scene))
    assert len(out) == 5 and all(o.grad_fn is None and not o.requires_grad for o in out)
    # a wrong device-side shape is refused by the binding before the library runs
    with pytest.raises(ValueError, match="shape"):
        GaussianRasterizer(util.hip_settings(scene, cam, D, DEV), index_maps=_index_maps(30, 41))


@pytest.mark.parametrize("size", [(40, 30), (7, 5)])
def test_edges_odd_image_sizes(size):
    W, H = size
    scene, cam, D = gsr_scene.make_scene(300, -2.5, sh_degree=1, seed=14), gsr_scene.make_camera(W, H), 1
    ups = _ups(H, W)
    for mode in MODES:
        r = direct(scene, cam, D, mode)
        n_last, n_before = check_definition(f"{W}x{H}/{mode}", r, scene, cam)
        assert n_last + n_before > 0
        f = fused(scene, cam, D, mode, ups, use_color=False)
        for k in ("med", "mi", "di", "dw"):
            assert torch.equal(f[k].reshape(r[k].shape), r[k]), k
        check_closed_form(f"{W}x{H}/{mode}", f["grads"], scene, cam, mode, f["mi"], ups[1])


# ---- 9. render() -----------------------------------------------------------------------------------------------------------------------------
def test_render_adds_median_depth_on_both_paths():
    """render(..., depth_alpha=, median_depth=True, index_maps=) puts the map into the dict and fills the caller's tensors on the
    activated path and on the leaf path (pipe.fused_activations): the first has the bits of GaussianRasterizer on the model's activated
    tensors, the second agrees with it the way test_renderer_gpu.py's alternates agree (a rounding of an activation may flip a
    threshold, and with it a pixel's median)."""
    import gsr_model
    from diff_gaussian_rasterization import GaussianRasterizer
    from gaussian_renderer import render
    scene, cam, D = _scene("B")
    P, H, W = scene.means3D.shape[0], cam.image_height, cam.image_width
    camd = cam._replace(world_view_transform=cam.world_view_transform.to(DEV), full_proj_transform=cam.full_proj_transform.to(DEV),
                        camera_center=cam.camera_center.to(DEV))
    g = _ups(H, W)[1]
    for kw in ({}, dict(fused_activations=True)):
        pc = gsr_model.GaussianParams.from_activated(scene.means3D, scene.shs, scene.scales, scene.rotations, scene.opacities, device=DEV,
                                                     max_sh_degree=D, active_sh_degree=D)
        ref_im = _index_maps(H, W)
        with torch.no_grad():
            ref = GaussianRasterizer(util.hip_settings(scene, cam, D, DEV), depth_alpha="depth", median_depth=True, index_maps=ref_im)(
                means3D=pc.get_xyz, means2D=torch.zeros(P, 3, device=DEV), opacities=pc.get_opacity, shs=pc.get_features,
                scales=pc.get_scaling, rotations=pc.get_rotation)
        im = _index_maps(H, W)
        r = render(camd, pc, gsr_model.pipeline_params(**kw), scene.bg.to(DEV), depth_alpha="depth", median_depth=True, index_maps=im)
        assert set(r) == {"render", "viewspace_points", "visibility_filter", "radii", "depth", "alpha", "median_depth"}
        assert r["median_depth"].shape == (1, H, W)
        if not kw:
            assert torch.equal(r["median_depth"].detach(), ref[4]) and torch.equal(r["render"].detach(), ref[0])
            for a, b in zip(im, ref_im):
                assert torch.equal(a, b)
        else:
            assert float((im[0] != ref_im[0]).float().mean()) < 1e-3 and float((im[1] != ref_im[1]).float().mean()) < 1e-3
            assert float(((r["median_depth"].detach() - ref[4]).abs() > 1e-5).float().mean()) < 1e-3
        (r["median_depth"] * g).sum().backward()
        assert float(pc._xyz.grad.abs().max()) > 0
        plain = render(camd, pc, gsr_model.pipeline_params(**kw), scene.bg.to(DEV), depth_alpha="depth")
        assert "median_depth" not in plain
        only = _index_maps(H, W)
        assert set(render(camd, pc, gsr_model.pipeline_params(**kw), scene.bg.to(DEV), index_maps=only)) == \
            {"render", "viewspace_points", "visibility_filter", "radii"}
        assert torch.equal(only[1], im[1])
        with pytest.raises(ValueError, match="depth_alpha"):
            render(camd, pc, gsr_model.pipeline_params(**kw), scene.bg.to(DEV), median_depth=True)
