"""GPU: the absolute screen-space gradients (include/gsr_absgrad.h, GaussianRasterizer(absgrad=(abs_mean2D, abs_gradient_accum)))
against the float64 per-pixel terms of tests/torch_splat_abs.py, with everything else the backward writes unchanged bit for bit; the
accumulator, the wave and run edges of the fold, a heavy tile walked in depth segments, and reference-free checks at size.

Bar per component (the rule of DESIGN 6b; a sum of moduli is its own sum |t|): |got - ref| <= max(1e-5 max_g ref, 3 d32), d32 the
distance of the helper's float32 run from its float64 run."""
import pytest
import torch

import __graft_entry__  # noqa: F401
import gsr_scene
import torch_splat_abs
import torch_splat_cam
import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cache = {}


def _cov_of(scene):
    """Sigma = R S^2 R^T in float64, rounded once."""
    P = scene.means3D.shape[0]
    r, x, y, z = scene.rotations.double().unbind(1)
    Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z),
                      1 - 2 * (x * x + z * z), 2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x),
                      1 - 2 * (x * x + y * y)], 1).reshape(P, 3, 3)
    M = Rm @ torch.diag_embed(scene.scales.double())
    S = M @ M.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).float()


def _terms(scene, cam, dL, colors=None, cov=None, D=3, o=None, **kw):
    o = util.oracle_forward(scene, cam, D, colors_precomp=colors, cov3D_precomp=cov, use_sh=colors is None,
                            use_scale_rot=cov is None) if o is None else o
    inputs = dict(means3D=scene.means3D, opacities=scene.opacities, V=cam.world_view_transform, PM=cam.full_proj_transform,
                  campos=cam.camera_center)
    if colors is None:
        inputs["shs"] = scene.shs
    else:
        kw["colors_precomp"] = colors
    if cov is None:
        inputs["scales"], inputs["rotations"] = scene.scales, scene.rotations
    else:
        kw["cov3D_precomp"] = cov
    return torch_splat_abs.abs_terms(o, inputs, dL, **kw)


def _reference(variant):
    """Scene, upstream gradients and the float64 terms of a variant of the camera test scene, computed once."""
    if variant in _cache:
        return _cache[variant]
    scene, cam = torch_splat_cam.camera_test_scene()
    P = scene.means3D.shape[0]
    g = torch.Generator().manual_seed(11)
    colors = torch.rand(P, 3, generator=g) if variant == "colors_precomp" else None
    cov = _cov_of(scene) if variant == "cov3D_precomp" else None
    o = util.oracle_forward(scene, cam, 3, colors_precomp=colors, cov3D_precomp=cov, use_sh=colors is None, use_scale_rot=cov is None)
    dpix = util.fragile_free_dpix(o, cam, seed=3)
    assert float((dpix == 0).all(0).float().mean()) < 0.05, "the scene zeroes too many fragile pixels"
    assert int((o["radii"] == 0).sum()) >= 10, "the scene lost its culled Gaussians"
    kw, dL = {}, dpix
    if variant in ("antialiasing", "aa_invdepth"):
        kw["antialiasing"] = True
    maps = lambda: (torch.randn(cam.image_height, cam.image_width, generator=g) * (dpix[0] != 0),
                    torch.randn(cam.image_height, cam.image_width, generator=g) * (dpix[0] != 0))
    if variant == "aa_invdepth":   # image and both maps in the loss
        kw["depth_mode"] = "invdepth"
        dL = (dpix,) + maps()
    if variant == "invdepth":      # through the maps alone
        kw["depth_mode"] = "invdepth"
        dL = (torch.zeros_like(dpix),) + maps()
    ref, signed, d32 = _terms(scene, cam, dL, colors, cov, o=o, **kw)
    assert torch_splat_abs.render.max_tiles == 6, "no splat covers every tile"
    assert torch_splat_abs.render.subpixel >= 1, "the scene lost its sub-pixel Gaussian"
    _cache[variant] = (scene, cam, colors, cov, dL, ref, signed, d32)
    return _cache[variant]


def _run(scene, cam, dL, absgrad="both", colors=None, cov=None, antialiasing=False, depth_alpha=None, camera_grads=False, D=3,
         debug=False, stats=True, backwards=1, accum_init=None):
    """One forward and `backwards` backwards on the GPU.  absgrad: None | "both" | "mean" | "accum".  -> dict"""
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device(DEV)
    leaf = lambda t: t.to(dev).clone().requires_grad_(True)
    P = scene.means3D.shape[0]
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
    st = util.hip_settings(scene, cam, D, dev, debug=debug)
    cams = [t.clone().requires_grad_(camera_grads) for t in (st.viewmatrix, st.projmatrix, st.campos)]
    st = st._replace(viewmatrix=cams[0], projmatrix=cams[1], campos=cams[2])
    # NaN / a marker in the outputs: the backward must overwrite every row of abs_mean2D and add into the accumulator
    am = torch.full((P, 2), float("nan"), device=dev) if absgrad in ("both", "mean") else None
    ac = (torch.zeros(P, device=dev) if accum_init is None else accum_init.to(dev).clone()) if absgrad in ("both", "accum") else None
    kw = {} if absgrad is None else dict(absgrad=(am, ac))
    dstats = tuple(torch.zeros(P, device=dev) for _ in range(3)) if stats else None
    out = GaussianRasterizer(st, antialiasing=antialiasing, depth_alpha=depth_alpha, densify_stats=dstats, camera_grads=camera_grads,
                             **kw)(**inp)
    if absgrad is not None and am is not None:
        assert bool(torch.isnan(am).all()), "the forward touched abs_mean2D"
    dL = dL if isinstance(dL, (tuple, list)) else (dL,)
    outs = (out[0],) + tuple(out[2:])
    loss = sum((o_ * d.to(dev).reshape(o_.shape)).sum() for o_, d in zip(outs, dL))
    res = dict(abs_first=None)
    for k in range(backwards):
        loss.backward(retain_graph=k + 1 < backwards)
        if k == 0 and backwards > 1:
            res["abs_first"] = (None if am is None else am.clone(), None if ac is None else ac.clone())
    torch.cuda.synchronize()
    res.update(image=out[0].detach(), radii=out[1], maps=[m.detach() for m in out[2:]], grads={k: v.grad for k, v in inp.items()},
               cams=[c.grad for c in cams], stats=dstats, abs_mean2D=am, accum=ac)
    return res


def _check(got, ref, d32, label):
    err = (got.detach().cpu().double() - ref).abs().max(0).values
    for c, name in enumerate("xy"):
        bar = max(1e-5 * float(ref[:, c].max()), 3 * float(d32[c]))
        line = f"absgrad {label} .{name}: err {float(err[c]):.3e} bar {bar:.3e} (max ref {float(ref[:, c].max()):.3e}, d32 {float(d32[c]):.3e})"
        print(line)
        util.parity_log(line)
        assert float(err[c]) <= bar, line


def _same_everything(a, b):
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["radii"], b["radii"])
    assert len(a["maps"]) == len(b["maps"]) and all(torch.equal(x, y) for x, y in zip(a["maps"], b["maps"]))
    assert a["grads"].keys() == b["grads"].keys()
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    if a["stats"] is not None:
        assert all(torch.equal(x, y) for x, y in zip(a["stats"], b["stats"]))


@pytest.mark.parametrize("variant", ["default", "colors_precomp", "cov3D_precomp", "antialiasing", "invdepth"])
def test_against_float64_terms_and_nothing_else_moves(variant):
    scene, cam, colors, cov, dL, ref, signed, d32 = _reference(variant)
    kw = dict(colors=colors, cov=cov, antialiasing=variant == "antialiasing", depth_alpha="invdepth" if variant == "invdepth" else None)
    a = _run(scene, cam, dL, "both", **kw)
    _check(a["abs_mean2D"], ref, d32, variant)
    culled = a["radii"] <= 0
    assert bool((a["abs_mean2D"][culled] == 0).all())
    b = _run(scene, cam, dL, None, **kw)
    _same_everything(a, b)
    assert float(b["stats"][0].abs().max()) > 0   # densify_stats stays what it was: signed


@pytest.mark.parametrize("variant", ["default", "aa_invdepth"])
def test_leaf_mode(variant):
    """Leaf mode alone, and leaf + anti-aliasing + inverse depth with image, D and A in the loss: the leaves are the inverse
    activations of the scene's tensors, so the blend sees the same function as the reference."""
    from fused_params import rasterize_leaf_gaussians
    scene, cam, _, _, dL, ref, signed, d32 = _reference(variant)
    kw = dict(depth_alpha="invdepth", antialiasing=True) if variant == "aa_invdepth" else {}
    dLs = dL if isinstance(dL, tuple) else (dL,)
    dev = torch.device(DEV)
    leaf = lambda t: t.to(dev).clone().requires_grad_(True)
    st = util.hip_settings(scene, cam, 3, dev)
    P = scene.means3D.shape[0]
    res = []
    for on in (True, False):
        op = scene.opacities.double()
        args = [leaf(scene.means3D), torch.zeros(scene.means3D.shape, device=dev, requires_grad=True), leaf(scene.shs[:, :1]),
                leaf(scene.shs[:, 1:]), leaf(torch.log(op / (1 - op)).float()), leaf(torch.log(scene.scales)), leaf(scene.rotations)]
        am, ac = torch.full((P, 2), float("nan"), device=dev), torch.zeros(P, device=dev)
        out = rasterize_leaf_gaussians(*args, st, absgrad=(am, ac) if on else None, **kw)
        sum((o_ * d.to(dev).reshape(o_.shape)).sum() for o_, d in zip((out[0],) + tuple(out[2:]), dLs)).backward()
        torch.cuda.synchronize()
        res.append((out, [a.grad for a in args], am, ac))
    _check(res[0][2], ref, d32, "leaf " + variant)
    vis = res[0][0][1] > 0
    torch.testing.assert_close(res[0][3][vis], torch.hypot(res[0][2][vis, 0], res[0][2][vis, 1]), rtol=1e-6, atol=0)
    for x, y in zip(res[0][0], res[1][0]):
        assert torch.equal(x, y)
    for x, y in zip(res[0][1], res[1][1]):
        assert torch.equal(x, y)


def test_camera_gradients_do_not_move():
    scene, cam, _, _, dL, ref, signed, d32 = _reference("default")
    a = _run(scene, cam, dL, "both", camera_grads=True)
    b = _run(scene, cam, dL, None, camera_grads=True)
    _check(a["abs_mean2D"], ref, d32, "camera_grads")
    _same_everything(a, b)
    assert all(x is not None and torch.equal(x, y) for x, y in zip(a["cams"], b["cams"]))


def test_accumulator_and_second_backward():
    scene, cam, _, _, dL, ref, *_ = _reference("default")
    init = torch.arange(scene.means3D.shape[0], dtype=torch.float32) * 0.25 + 1.0
    a = _run(scene, cam, dL, "both", accum_init=init, backwards=2)
    vis = (a["radii"] > 0)
    norm = torch.hypot(a["abs_mean2D"][:, 0], a["abs_mean2D"][:, 1])
    first_m, first_a = a["abs_first"]
    assert torch.equal(first_m, a["abs_mean2D"])   # overwritten with the same bits
    assert torch.equal(first_a[~vis], init.to(DEV)[~vis]) and torch.equal(a["accum"][~vis], init.to(DEV)[~vis])
    inc1 = (first_a - init.to(DEV))[vis].double()
    torch.testing.assert_close(inc1, norm[vis].double(), rtol=1e-6, atol=float(torch.finfo(torch.float32).eps * init.max()))
    inc2 = (a["accum"] - init.to(DEV))[vis].double()
    torch.testing.assert_close(inc2, 2 * norm[vis].double(), rtol=1e-6, atol=2 * float(torch.finfo(torch.float32).eps * (init.max() + 2 * norm.max())))
    # from zero the increment is the norm itself to a few ulp
    z = _run(scene, cam, dL, "both")
    torch.testing.assert_close(z["accum"][vis], norm[vis], rtol=1e-6, atol=0)
    assert bool((z["accum"][~vis] == 0).all())


def test_only_one_tensor_given():
    scene, cam, _, _, dL, *_ = _reference("default")
    both = _run(scene, cam, dL, "both")
    m = _run(scene, cam, dL, "mean")
    c = _run(scene, cam, dL, "accum")
    assert m["accum"] is None and c["abs_mean2D"] is None
    assert torch.equal(m["abs_mean2D"], both["abs_mean2D"]) and torch.equal(c["accum"], both["accum"])
    _same_everything(m, both)
    _same_everything(c, both)


def test_no_grad_and_no_backward_touch_nothing():
    from diff_gaussian_rasterization import GaussianRasterizer
    scene, cam = torch_splat_cam.camera_test_scene()
    dev = torch.device(DEV)
    P = scene.means3D.shape[0]
    am, ac = torch.full((P, 2), 7.0, device=dev), torch.full((P,), 3.0, device=dev)
    with torch.no_grad():
        GaussianRasterizer(util.hip_settings(scene, cam, 3, dev), absgrad=(am, ac))(
            means3D=scene.means3D.to(dev), means2D=torch.zeros(P, 3, device=dev), opacities=scene.opacities.to(dev),
            shs=scene.shs.to(dev), scales=scene.scales.to(dev), rotations=scene.rotations.to(dev))
    torch.cuda.synchronize()
    assert bool((am == 7.0).all()) and bool((ac == 3.0).all())


def test_one_pixel_image():
    """1 x 1: every sum has one term, so abs_mean2D is |dL/dmean2D| -- formed by different roundings, hence not bit-equal."""
    scene, cam = gsr_scene.make_scene(40, -1.0, sh_degree=3, seed=6), gsr_scene.make_camera(1, 1)
    a = _run(scene, cam, torch.tensor([0.7, -1.3, 0.4]).reshape(3, 1, 1), "both")
    signed = a["grads"]["means2D"][:, :2].abs()
    assert float(signed.max()) > 0
    assert float((a["abs_mean2D"] - signed).abs().max()) <= 1e-5 * float(signed.max())


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65])
def test_wave_edges(P):
    scene, cam = gsr_scene.make_scene(P, -1.0, sh_degree=3, seed=2), gsr_scene.make_camera(40, 24)
    dpix = torch.randn(3, 24, 40, generator=torch.Generator().manual_seed(1))
    a = _run(scene, cam, dpix, "both")
    assert a["abs_mean2D"].shape == (P, 2) and not bool(torch.isnan(a["abs_mean2D"]).any())
    if P == 0:
        return
    signed = a["grads"]["means2D"][:, :2].abs()
    assert bool((a["abs_mean2D"] >= signed - 1e-5 * float(signed.max())).all())
    if P >= 63:
        assert float(a["abs_mean2D"].max()) > 0
    _same_everything(a, _run(scene, cam, dpix, None))


def test_all_culled_scene_gives_exact_zeros():
    scene, cam = gsr_scene.make_scene(130, -1.0, sh_degree=3, seed=2), gsr_scene.make_camera(40, 24)
    scene = scene._replace(means3D=scene.means3D - torch.tensor([0.0, 0.0, 20.0]))   # all behind the camera
    a = _run(scene, cam, torch.ones(3, 24, 40), "both", accum_init=torch.full((130,), 2.0))
    assert bool((a["abs_mean2D"] == 0).all()) and bool((a["accum"] == 2.0).all())


def test_only_the_last_lane_of_the_last_wave_is_visible():
    scene, cam = gsr_scene.make_scene(128, -1.0, sh_degree=3, seed=4), gsr_scene.make_camera(40, 24)
    means = scene.means3D - torch.tensor([0.0, 0.0, 20.0])
    means[127] = torch.tensor([0.1, -0.05, 0.2])
    scene = scene._replace(means3D=means)
    dpix = torch.randn(3, 24, 40, generator=torch.Generator().manual_seed(1))
    a = _run(scene, cam, dpix, "both")
    assert bool((a["abs_mean2D"][:127] == 0).all()) and float(a["abs_mean2D"][127].min()) > 0
    assert bool((a["accum"][:127] == 0).all()) and float(a["accum"][127]) > 0


def test_run_longer_than_the_cooperative_threshold():
    """128 x 96 (48 tiles): one Gaussian covers every tile, so the whole wave folds its run (more than GSR_SLOT_COOP = 30 slots)."""
    scene, cam = gsr_scene.make_scene(24, -2.0, sh_degree=3, seed=12), gsr_scene.make_camera(128, 96)
    scales, means = scene.scales.clone(), scene.means3D.clone()
    scales[5] = 2.0
    means[5] = torch.tensor([0.05, 0.02, 0.6])
    scene = scene._replace(scales=scales, means3D=means)
    o = util.oracle_forward(scene, cam, 3)
    assert int(o["tiles_touched"][5]) == 48
    dpix = util.fragile_free_dpix(o, cam, seed=5)
    assert float((dpix == 0).all(0).float().mean()) < 0.05
    ref, signed, d32 = _terms(scene, cam, dpix, o=o)
    a = _run(scene, cam, dpix, "both")
    _check(a["abs_mean2D"], ref, d32, "48-tile run")
    assert float(a["abs_mean2D"][5].min()) > 0
    _same_everything(a, _run(scene, cam, dpix, None))


def _heavy_scene():
    """The construction of test_boundary_gpu._heavy_scene at a size the dense helper takes.  The backward cuts tiles in depth only
    from 64 tiles on (binning.hip gsr_tile_order_max_segments), so the image is a strip of 64 tiles, 1024 x 4, and a low-opacity blob
    of 1 300 small Gaussians sits in the middle of tile 32: the opacities are too low to end the walk, so what the binning lists
    there is walked to the end, more than two checkpoint strides (2 x 512 list positions) deep."""
    P, W, H, D = 1300, 1024, 4, 1
    scene = gsr_scene.make_scene(P, -5.0, sh_degree=D, seed=9)
    g = torch.Generator().manual_seed(10)
    # 234 pixels per unit at the blob's depth: 3.5 x 1 pixels of spread around the centre of tile 32 (pixel 520)
    means = torch.randn(P, 3, generator=g) * torch.tensor([0.015, 0.004, 0.3]) + torch.tensor([0.034, 0.0, 0.0])
    opac = torch.sigmoid(torch.randn(P, 1, generator=g) - 4.5)
    return scene._replace(means3D=means.contiguous(), opacities=opac.contiguous()), gsr_scene.make_camera(W, H), D


def _depth_segments(scene, cam, D, dpix, absgrad):
    """One forward and one absgrad backward through the extension's functions, to read the backward's dispatch list out of the image
    state (test_boundary_gpu.test_heavy_tiles_split_in_bands_and_in_depth reads it the same way).
    -> (tiles cut in depth, segment entries, coarseness, tiles the forward split in bands, deepest walk)"""
    from diff_gaussian_rasterization import _C
    dev = torch.device(DEV)
    W, H = cam.image_width, cam.image_height
    st = util.hip_settings(scene, cam, D, dev)
    e = torch.empty(0, device=dev)
    t = {k: getattr(scene, k).to(dev) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    R, color, radii, geom, binning, img = _C.rasterize_gaussians(st.bg, t["means3D"], e, t["opacities"], t["scales"], t["rotations"], 1.0, e,
                                                                 st.viewmatrix, st.projmatrix, st.tanfovx, st.tanfovy, H, W, t["shs"], D,
                                                                 st.campos, False, False)
    T = ((W + 15) // 16) * ((H + 15) // 16)
    il = _C.image_layout(W, H)

    def entries(count):
        v = img[il.tile_order:il.tile_order + 4 * count].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        return v[v != 0xFFFFFFFF]
    nbands = int((entries(T + 3 * min(2048, T // 4)) >> 28 > 0).sum())
    rng = img[il.ranges:il.ranges + 8 * T].view(torch.int32).view(T, 2)
    lens = (rng[:, 1] - rng[:, 0]).to(torch.int64)
    tmc = img[il.tile_max_contrib:il.tile_max_contrib + 4 * T].view(torch.int32).to(torch.int64)
    walked = torch.minimum(lens, tmc)
    _C.rasterize_gaussians_backward(st.bg, t["means3D"], radii, e, t["scales"], t["rotations"], 1.0, e, st.viewmatrix, st.projmatrix, st.tanfovx,
                                    st.tanfovy, dpix.to(dev), t["shs"], D, st.campos, geom, R, binning, img, False, absgrad=absgrad)
    torch.cuda.synchronize()
    budget = min(4096, T // 2)
    valid = entries(T + budget)
    seg, tiles = valid >> 28, valid & 0x0FFFFFFF
    cut = torch.unique(tiles[seg > 0])
    coarse = int(img[il.tile_order + 4 * (T + budget):il.tile_order + 4 * (T + budget) + 4].view(torch.int32)[0])
    assert coarse in (1, 2, 4, 8) and cut.numel() >= 1, "no tile was cut in depth"
    assert torch.equal(torch.sort(cut).values, torch.nonzero(walked >= (coarse + 1) * 512).flatten())   # (GSR_CKPT_STRIDE = 512 list positions)
    assert valid.numel() == T + int((seg > 0).sum()) - cut.numel()
    return cut.numel(), int((seg > 0).sum()), coarse, nbands // 4, int(walked.max())


def test_heavy_tile_split_and_unsplit():
    """The ABS blend over depth segments: every instance is walked by exactly one segment wave, which starts from the forward's
    (T, C) checkpoint, so f -- and with it every modulus -- agrees with the unsplit walk to rounding only.  Both runs sit inside the
    bar against the helper, and the split must actually have happened: the backward's dispatch list holds segment entries."""
    from diff_gaussian_rasterization import _C
    scene, cam, D = _heavy_scene()
    P = scene.means3D.shape[0]
    o = util.oracle_forward(scene, cam, D)
    assert int(o["n_contrib"].max()) >= 1024, "no tile is walked two checkpoint strides deep"
    dpix = util.fragile_free_dpix(o, cam, seed=2)
    assert float((dpix == 0).all(0).float().mean()) < 0.05
    ref, signed, d32 = _terms(scene, cam, dpix, D=D, o=o)
    split = _run(scene, cam, dpix, "both", D=D)
    whole = _run(scene, cam, dpix, "both", D=D, debug=_C.DEBUG_NO_SPLIT)
    _check(split["abs_mean2D"], ref, d32, "heavy tile, depth segments")
    _check(whole["abs_mean2D"], ref, d32, "heavy tile, GSR_DEBUG_NO_SPLIT")
    _same_everything(split, _run(scene, cam, dpix, None, D=D))
    # the dispatch list of the same backward, called directly: segment entries, and the bits of the run checked above
    am, ac = torch.full((P, 2), float("nan"), device=DEV), torch.zeros(P, device=DEV)
    ncut, nseg, coarse, nband, deepest = _depth_segments(scene, cam, D, dpix, (am, ac))
    assert ncut >= 1 and nseg >= 2 * ncut
    assert torch.equal(am, split["abs_mean2D"]) and torch.equal(ac, split["accum"])
    dist = (split["abs_mean2D"] - whole["abs_mean2D"]).abs().max(0).values / split["abs_mean2D"].max(0).values
    line = (f"absgrad heavy tile: {ncut} of 64 tiles cut in depth into {nseg} segments (coarseness {coarse}, deepest walk {deepest}), "
            f"{nband} split in bands by the forward; split vs GSR_DEBUG_NO_SPLIT {float(dist[0]):.2e} / {float(dist[1]):.2e} of the largest")
    print(line)
    util.parity_log(line)


@pytest.mark.parametrize("P", [20_011, 100_003])
def test_at_size_reference_free(P):
    from diff_gaussian_rasterization import _C
    scene, cam = gsr_scene.make_scene(P, -2.5, sh_degree=3, seed=9), gsr_scene.make_camera(128, 96)
    scales = scene.scales.clone()
    scales[:3] = 2.0
    scene = scene._replace(scales=scales)
    dpix = torch.randn(3, 96, 128, generator=torch.Generator().manual_seed(2))
    a = _run(scene, cam, dpix, "both")
    signed = a["grads"]["means2D"][:, :2].abs()
    assert bool((a["abs_mean2D"] >= signed - 1e-5 * float(a["abs_mean2D"].max())).all())
    assert float((a["abs_mean2D"].sum(1) / signed.sum(1).clamp_min(1e-30)).max()) > 10   # cancellation is what it is for
    again = _run(scene, cam, dpix, "both")
    assert torch.equal(a["abs_mean2D"], again["abs_mean2D"]) and torch.equal(a["accum"], again["accum"])
    _same_everything(a, _run(scene, cam, dpix, None))
    runs = {}
    for flag in ("DEBUG_NO_TRIM", "DEBUG_NO_SPLIT"):
        r1 = _run(scene, cam, dpix, "both", debug=getattr(_C, flag))
        r2 = _run(scene, cam, dpix, "both", debug=getattr(_C, flag))
        assert torch.equal(r1["abs_mean2D"], r2["abs_mean2D"]) and torch.equal(r1["accum"], r2["accum"]), flag
        runs[flag] = r1
    # trimmed instances hold no hit: the untrimmed lists give the same bits
    assert torch.equal(a["abs_mean2D"], runs["DEBUG_NO_TRIM"]["abs_mean2D"]) and torch.equal(a["accum"], runs["DEBUG_NO_TRIM"]["accum"])


def test_view_parallel_raises():
    import view_parallel
    with pytest.raises(NotImplementedError, match="absgrad"):
        view_parallel.rasterize_view_parallel(*([None] * 8), absgrad=(torch.zeros(4, 2, device=DEV), None))


@pytest.mark.parametrize("fused", [False, True])
def test_render_reaches_the_tensors(fused):
    import gsr_model
    from gaussian_renderer import render
    dev = torch.device(DEV)
    scene, cam = torch_splat_cam.camera_test_scene()
    P = scene.means3D.shape[0]
    pc = gsr_model.GaussianParams.from_activated(scene.means3D, scene.shs, scene.scales, scene.rotations, scene.opacities,
                                                 device=dev, active_sh_degree=3)
    camd = cam._replace(world_view_transform=cam.world_view_transform.to(dev), full_proj_transform=cam.full_proj_transform.to(dev),
                        camera_center=cam.camera_center.to(dev))
    am, ac = torch.full((P, 2), float("nan"), device=dev), torch.zeros(P, device=dev)
    out = render(camd, pc, gsr_model.pipeline_params(fused_activations=fused), scene.bg.to(dev), absgrad=(am, ac))
    g = torch.Generator().manual_seed(3)
    (out["render"] * torch.randn(3, cam.image_height, cam.image_width, generator=g).to(dev)).sum().backward()
    torch.cuda.synchronize()
    vis = out["radii"] > 0
    signed = out["viewspace_points"].grad[:, :2].abs()
    assert not bool(torch.isnan(am).any()) and bool((am[~vis] == 0).all()) and float(am.max()) > 0
    assert bool((am >= signed - 1e-5 * float(am.max())).all())
    torch.testing.assert_close(ac[vis], torch.hypot(am[vis, 0], am[vis, 1]), rtol=1e-6, atol=0)
