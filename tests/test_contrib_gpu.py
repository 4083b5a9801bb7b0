"""GPU: per-Gaussian blend-weight statistics (include/gsr_contrib.h; _C.gaussian_contributions, GaussianRasterizer(contrib_stats=...)).

The reference is the float64 walk below over the run's OWN state (util.unpack_state: the records' means2D and conic_opacity,
point_list, ranges, n_contrib -- intermediates the parity tests pin against the oracle): per tile and per list position
j < n_contrib[p] it evaluates power, alpha, the two thresholds, w = alpha T and T *= 1 - alpha.

Fragile pairs: |255 alpha - 1| < 1e-3 or |power| < 1e-5 -- an fp32 evaluation may decide them the other way.  A pixel is tainted from its
first fragile pair on: its later T may differ by the factor the flipped pair applies.  A tainted stretch holds the fragile pairs (hit in the
reference or not, with w = alpha T as for a hit) and every later hit of the pixel.  Per Gaussian the walk gives sum_ref, the counts
without and with the fragile pairs (count_lo, count_hi), the largest reference w over untainted pairs (max_lo) and over all pairs,
tainted stretches included (max_hi), and two slacks:
  slack_lit  the sum of m w over its pairs inside tainted stretches;
  slack      the same for a fragile pair; for a later pair the smaller of its m w and m (w_up - w_low), with w_up = alpha T_up taken with the largest T either decision can
             leave (no fragile pair applied) and w_low with the smallest (all applied).  By construction slack <= slack_lit.
The sum is asserted with `slack`, never with more than slack_lit allows, and the maximum against max_hi, the reference's own w.  The
slack is kept from hiding a failure by two conditions asserted on the reference: tainted pixels are at most 5 % of the image, Gaussians
with slack > 1 % of their sum at most 10 % of the contributing ones.  The second condition is why `slack` and not slack_lit is the bar:
slack_lit fails it on the reference itself, before any kernel runs -- a pixel behind a fragile pair holds some 30 more Gaussians, most
of them a few pixels large, so one tainted pixel is a large share of each one's sum (the test prints both figures; on the CPU oracle's state, m = 1:
slack_lit > 1 % of the sum for 283 of A's 1 776 contributing Gaussians, 15.9 %, and 678 of B's 2 933, 23.1 %; `slack` for 3 and 1).  A pair behind a flipped fragile pair moves by the factor (1 - alpha_f) or its inverse, 0.4 % of w
for alpha_f = 1 / 255, which m (w_up - w_low) covers and the whole m w overstates 250-fold; only behind a flipped |power| < 1e-5 pair
with alpha_f > 0.5 can the move exceed w, and there `slack` stays at the smaller m w.

Shapes: A = make_scene(2000, -3.0, sh_degree=1, seed=33) at 33 x 17 (a one-pixel tile column and a one-pixel tile row; longest list
1 188 >= 2 * GSR_CKPT_STRIDE: a heavy tile, band-split forward, many batches), B = make_scene(3000, -3.0, sh_degree=1, seed=21) at
120 x 90 (48 tiles, 11 977 instances), C = nothing to do (P = 0, one Gaussian, a scene behind the camera)."""
import functools

import numpy as np
import pytest
import torch

import gsr_scene
import util

pytestmark = pytest.mark.gpu

SCENES = {"A": (2000, 33, 33, 17), "B": (3000, 21, 120, 90)}   # P, seed, W, H
D = 1


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def ref_walk(st, W, H, m=None):
    """The float64 reference (module docstring).  st: util.unpack_state's dict (or the oracle's); m: (H, W) weights or None."""
    xy, co = st["means2D"].astype(np.float64), st["conic_opacity"].astype(np.float64)
    P = xy.shape[0]
    plist, ranges, n_contrib = st["point_list"].astype(np.int64), st["ranges"].astype(np.int64), st["n_contrib"].astype(np.int64)
    mflat = np.ones(W * H) if m is None else np.asarray(m, np.float64).reshape(-1)
    r = dict(sum=np.zeros(P), slack=np.zeros(P), slack_lit=np.zeros(P), max_lo=np.zeros(P), max_hi=np.zeros(P), count_lo=np.zeros(P, np.int64),
             count_hi=np.zeros(P, np.int64), pairs=0, fragile=0, tainted_pixels=0)
    gx = (W + 15) // 16
    for t in range(ranges.shape[0]):
        a, b = ranges[t]
        if b <= a:
            continue
        ys, xs = np.meshgrid(np.arange(16 * (t // gx), min(H, 16 * (t // gx) + 16)), np.arange(16 * (t % gx), min(W, 16 * (t % gx) + 16)), indexing="ij")
        pix = (ys * W + xs).reshape(-1)
        px, py, nc, mm = xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64), n_contrib[pix], mflat[pix]
        T, Tup, Tlow, taint = np.ones(pix.size), np.ones(pix.size), np.ones(pix.size), np.zeros(pix.size, bool)
        for j in range(int(min(b - a, nc.max()))):
            g = plist[a + j]
            dx, dy = xy[g, 0] - px, xy[g, 1] - py
            power = -0.5 * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
            alpha = np.minimum(0.99, co[g, 3] * np.exp(np.minimum(power, 50.0)))
            act = j < nc
            frag = act & ((np.abs(255.0 * alpha - 1.0) < 1e-3) | (np.abs(power) < 1e-5))
            hit = act & ~(power > 0.0) & ~(alpha < 1.0 / 255.0)
            taint |= frag
            clean = hit & ~taint
            dirty = taint & (hit | frag)
            w, wup, wlow = alpha * T, alpha * Tup, alpha * Tlow
            r["sum"][g] += float((mm * w)[hit].sum())
            r["slack_lit"][g] += float((mm * w)[dirty].sum())
            r["slack"][g] += float((mm * np.where(frag, w, np.minimum(w, wup - wlow)))[dirty].sum())
            r["count_lo"][g] += int((hit & ~frag).sum())
            r["count_hi"][g] += int((hit | frag).sum())
            r["max_lo"][g] = max(r["max_lo"][g], float(w[clean].max(initial=0.0)))
            r["max_hi"][g] = max(r["max_hi"][g], float(w[hit | frag].max(initial=0.0)))
            r["pairs"] += int(hit.sum())
            r["fragile"] += int(frag.sum())
            T = np.where(hit, T * (1.0 - alpha), T)
            Tup = np.where(hit & ~frag, Tup * (1.0 - alpha), Tup)
            Tlow = np.where(hit | frag, Tlow * (1.0 - alpha), Tlow)
        r["tainted_pixels"] += int(taint.sum())
    return r


def _dev():
    return torch.device("cuda:0")


def _forward(scene, cam, debug=0, colors=None, antialiasing=False):
    """_C.rasterize_gaussians on cuda:0 -> (R, color, radii, geom, binning, img) and the device inputs."""
    from diff_gaussian_rasterization import _C
    dev = _dev()
    to = lambda t: t.to(dev).contiguous()
    e = torch.empty(0, device=dev)
    inp = dict(bg=to(scene.bg), means3D=to(scene.means3D), colors=e if colors is None else to(colors), opacities=to(scene.opacities),
               scales=to(scene.scales), rotations=to(scene.rotations), view=to(cam.world_view_transform), proj=to(cam.full_proj_transform),
               shs=to(scene.shs) if colors is None else e, campos=to(cam.camera_center))
    r = _C.rasterize_gaussians(inp["bg"], inp["means3D"], inp["colors"], inp["opacities"], inp["scales"], inp["rotations"], 1.0, e, inp["view"],
                               inp["proj"], cam.tanfovx, cam.tanfovy, cam.image_height, cam.image_width, inp["shs"], D, inp["campos"], False,
                               debug, antialiasing=antialiasing)
    return r, inp


def _backward(r, inp, cam, dpix):
    from diff_gaussian_rasterization import _C
    e = torch.empty(0, device=_dev())
    return _C.rasterize_gaussians_backward(inp["bg"], inp["means3D"], r[2], inp["colors"], inp["scales"], inp["rotations"], 1.0, e, inp["view"],
                                           inp["proj"], cam.tanfovx, cam.tanfovy, dpix, inp["shs"], D, inp["campos"], r[3], r[0], r[4], r[5], False)


def _stats(P, fill=(0.0, 0.0, 0)):
    dev = _dev()
    return (torch.full((P,), fill[0], dtype=torch.float32, device=dev), torch.full((P,), fill[1], dtype=torch.float32, device=dev),
            torch.full((P,), fill[2], dtype=torch.int32, device=dev))


def _contrib(r, P, cam, m=None, debug=0, fill=(0.0, 0.0, 0)):
    """-> (weight_sum, weight_max, pixel_count) as numpy, from tensors pre-filled with `fill`"""
    from diff_gaussian_rasterization import _C
    s = _stats(P, fill)
    _C.gaussian_contributions(r[3], r[4], r[5], r[0], P, cam.image_width, cam.image_height, s, m, debug)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in s)


def _weight_map(W, H):
    return torch.rand(H, W, generator=torch.Generator().manual_seed(5)) * 1.5 + 0.25   # positive, in [0.25, 1.75)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The default forward of scene A / B, its unpacked state, and the reference walks without and with the weight map (computed once,
    shared by the tests, never modified)."""
    P, seed, W, H = SCENES[name]
    scene, cam = gsr_scene.make_scene(P, -3.0, sh_degree=D, seed=seed), gsr_scene.make_camera(W, H)
    r, inp = _forward(scene, cam)
    torch.cuda.synchronize()
    st = util.unpack_state(dict(R=r[0], geom=r[3], binning=r[4], img=r[5]), P, W, H)
    m = _weight_map(W, H)
    return dict(P=P, W=W, H=H, scene=scene, cam=cam, r=r, inp=inp, st=st, m=m, ref={False: ref_walk(st, W, H), True: ref_walk(st, W, H, m.numpy())})


def _check_against(ref, got, npix, label, guard=True):
    ws, wm, pc = (x.astype(np.float64) for x in got)
    contributing = ref["count_hi"] > 0
    # the slack must not be what passes the test
    loose = (ref["slack"] > 0.01 * ref["sum"]) & contributing
    if guard:
        assert ref["tainted_pixels"] <= 0.05 * npix, (label, ref["tainted_pixels"], npix)
        assert loose.sum() <= 0.10 * contributing.sum(), (label, int(loose.sum()), int(contributing.sum()))
    err = np.abs(ws - ref["sum"])
    bar = 1e-5 * ref["sum"] + ref["slack"] + 1e-7
    loose_lit = (ref["slack_lit"] > 0.01 * ref["sum"]) & contributing
    assert bool((ref["slack"] <= ref["slack_lit"] * (1 + 1e-12)).all()), label   # never more than the issue's reading allows
    tight = ref["max_hi"] > 0
    print(f"{label}: pairs {ref['pairs']} fragile {ref['fragile']} tainted pixels {ref['tainted_pixels']} contributing {int(contributing.sum())} "
          f"with slack {int((ref['slack'] > 0).sum())} loose {int(loose.sum())} (with slack_lit: {int(loose_lit.sum())}); "
          f"worst sum err / bar {float((err / bar).max()):.3f}, "
          f"worst without slack {float((err[ref['slack'] == 0] / bar[ref['slack'] == 0]).max(initial=0.0)):.3f}; "
          f"worst weight_max / max_hi - 1 = {float((wm[tight] / ref['max_hi'][tight]).max(initial=1.0) - 1.0):.3e}, "
          f"worst 1 - weight_max / max_lo = {float(1.0 - (wm[ref['max_lo'] > 0] / ref['max_lo'][ref['max_lo'] > 0]).min(initial=1.0)):.3e}")
    assert bool((pc >= ref["count_lo"]).all()) and bool((pc <= ref["count_hi"]).all()), label
    assert bool((err <= bar).all()), (label, float((err / bar).max()))
    assert bool((wm >= ref["max_lo"] * (1 - 1e-5)).all()) and bool((wm <= ref["max_hi"] * (1 + 1e-5)).all()), label


@pytest.mark.parametrize("name", ["A", "B"])
def test_against_the_float64_walk(name):
    """Assertion 1: counts, sums and maxima against the reference, without and with a weight map; Gaussians without a pair keep the
    pre-filled values; weight_max and pixel_count do not depend on the map."""
    _need_gpu()
    c = _case(name)
    P, W, H, cam = c["P"], c["W"], c["H"], c["cam"]
    lens = c["st"]["ranges"].astype(np.int64)
    if name == "A":
        assert int((lens[:, 1] - lens[:, 0]).max()) >= 1024, "scene A no longer has a heavy tile"
    plain = _contrib(c["r"], P, cam)
    mapped = _contrib(c["r"], P, cam, c["m"].to(_dev()))
    _check_against(c["ref"][False], plain, W * H, f"contrib {name} m=1")
    _check_against(c["ref"][True], mapped, W * H, f"contrib {name} map")
    assert np.array_equal(plain[1].view(np.uint32), mapped[1].view(np.uint32)) and np.array_equal(plain[2], mapped[2])
    mapped3 = _contrib(c["r"], P, cam, c["m"].to(_dev()).reshape(1, H, W))
    assert np.array_equal(mapped[0].view(np.uint32), mapped3[0].view(np.uint32))
    # sentinels: a Gaussian the reference gives no pair is untouched, and exactly the Gaussians with a hit are written
    sent = _contrib(c["r"], P, cam, fill=(-3.0, -1.0, -5))
    none = c["ref"][False]["count_hi"] == 0
    assert none.any() and bool((sent[0][none] == -3.0).all()) and bool((sent[1][none] == -1.0).all()) and bool((sent[2][none] == -5).all())
    assert np.array_equal(sent[2] != -5, plain[2] > 0) and np.array_equal(sent[2][plain[2] > 0], plain[2][plain[2] > 0] - 5)
    assert np.array_equal(sent[1][plain[2] > 0], plain[1][plain[2] > 0])   # max(-1, mx) = mx


@pytest.mark.parametrize("name", ["A", "B"])
def test_sums_telescope_to_one_minus_final_T(name):
    """Assertion 2, reference-free: with m = 1 the weights of a pixel sum to 1 - T_final, so do all of them over the image."""
    _need_gpu()
    c = _case(name)
    ws = _contrib(c["r"], c["P"], c["cam"])[0]
    total, want = float(ws.astype(np.float64).sum()), float((1.0 - c["st"]["final_T"].astype(np.float64)).sum())
    util.parity_log(f"contrib {name}: sum_g weight_sum = {total:.9g}, sum_p (1 - final_T) = {want:.9g}, rel diff {abs(total - want) / want:.3e} (bar 1e-5)")
    assert abs(total - want) <= 1e-5 * want, (total, want)


def test_weight_sum_equals_the_colour_gradient_of_the_backward():
    """Assertion 3 (B): with colors_precomp and dL/dpix = m in every channel, dL/dcolors[:, 0] is the same sum of m w."""
    _need_gpu()
    c = _case("B")
    P, W, H, cam = c["P"], c["W"], c["H"], c["cam"]
    colors = torch.rand(P, 3, generator=torch.Generator().manual_seed(9))
    r, inp = _forward(c["scene"], cam, colors=colors)
    m = c["m"].to(_dev())
    ws = _contrib(r, P, cam, m)[0].astype(np.float64)
    dc = _backward(r, inp, cam, m.expand(3, H, W).contiguous())[1][:, 0].cpu().numpy().astype(np.float64)
    ratio = np.abs(ws - dc) / (1e-5 * dc + 1e-7)
    util.parity_log(f"contrib B: weight_sum vs dL/dcolors[:, 0] of the backward, worst |diff| / (1e-5 rel + 1e-7) = {float(ratio.max()):.3f}")
    print(f"worst ratio {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0


def _bits(got):
    return tuple(x.view(np.uint32) if x.dtype == np.float32 else x for x in got)


@pytest.mark.parametrize("name", ["A", "B"])
def test_bit_identical_across_runs_and_debug_switches(name):
    """Assertion 4: a second call, GSR_DEBUG_NO_CULL, a GSR_DEBUG_NO_TRIM forward and (A) a GSR_DEBUG_NO_SPLIT forward."""
    _need_gpu()
    from diff_gaussian_rasterization import _C
    c = _case(name)
    P, cam, m = c["P"], c["cam"], c["m"].to(_dev())
    base = _bits(_contrib(c["r"], P, cam, m))
    variants = {"again": _contrib(c["r"], P, cam, m), "no_cull": _contrib(c["r"], P, cam, m, debug=_C.DEBUG_NO_CULL),
                "no_trim": _contrib(_forward(c["scene"], cam, debug=_C.DEBUG_NO_TRIM)[0], P, cam, m)}
    if name == "A":
        variants["no_split"] = _contrib(_forward(c["scene"], cam, debug=_C.DEBUG_NO_SPLIT)[0], P, cam, m)
    for label, got in variants.items():
        for x, y in zip(base, _bits(got)):
            assert np.array_equal(x, y), (name, label)


def test_accumulation_over_two_views():
    """Assertion 5: two views into the same tensors = the sum (weight_sum, pixel_count) / the max (weight_max) of the single views,
    and the three statistics stand in the relations their definitions imply."""
    _need_gpu()
    from diff_gaussian_rasterization import _C
    P, seed, W, H = SCENES["B"]
    scene = gsr_scene.make_scene(P, -3.0, sh_degree=D, seed=seed)
    acc, single = _stats(P), []
    for k in (0, 1):
        cam = gsr_scene.ring_camera(W, H, k)
        r, _ = _forward(scene, cam)
        _C.gaussian_contributions(r[3], r[4], r[5], r[0], P, W, H, acc)
        single.append(_contrib(r, P, cam))
    torch.cuda.synchronize()
    ws, wm, pc = (t.cpu().numpy() for t in acc)
    assert np.array_equal(ws, single[0][0] + single[1][0])   # 0 + a + b in fp32: the same two roundings
    assert np.array_equal(wm, np.maximum(single[0][1], single[1][1])) and np.array_equal(pc, single[0][2] + single[1][2])
    assert (single[0][2] > 0).any() and (single[1][2] > 0).any() and not np.array_equal(single[0][2], single[1][2])
    for s, x, n in single + [(ws, wm, pc)]:
        assert np.array_equal(n > 0, x > 0) and float(x.max()) <= 0.99
    for s, x, n in single:   # m = 1, one view
        assert bool((x <= s).all()) and bool((s.astype(np.float64) <= n * x.astype(np.float64) * (1 + 1e-6)).all())


def test_the_pass_leaves_the_state_and_the_backward_alone():
    """Assertion 6 (A): the three state buffers are byte-identical before and after the pass, and forward -> pass -> backward gives the
    gradients of forward -> backward bit for bit."""
    _need_gpu()
    c = _case("A")
    P, W, H, cam, scene = c["P"], c["W"], c["H"], c["cam"], c["scene"]
    dpix = torch.randn(3, H, W, generator=torch.Generator().manual_seed(3)).to(_dev())
    r1, inp1 = _forward(scene, cam)
    g1 = _backward(r1, inp1, cam, dpix)
    r2, inp2 = _forward(scene, cam)
    before = [r2[k].clone() for k in (3, 4, 5)]
    got = _contrib(r2, P, cam, c["m"].to(_dev()))
    assert int((got[2] > 0).sum()) > 0
    for b, k in zip(before, (3, 4, 5)):
        assert torch.equal(b, r2[k]), f"state buffer {k} changed"
    g2 = _backward(r2, inp2, cam, dpix)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)


def _module_run(c, contrib, **opts):
    """GaussianRasterizer(...) under no_grad with the forward's state captured -> (outputs, captured forward result)."""
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    inp = c["inp"]
    settings = util.hip_settings(c["scene"], c["cam"], D, _dev())
    cap = {}
    names = ("rasterize_gaussians", "rasterize_gaussians_depth_alpha")
    orig = {n: getattr(_C, n) for n in names}

    def spy(n):
        def f(*a, **kw):
            cap["r"] = orig[n](*a, **kw)
            return cap["r"]
        return f
    for n in names:
        setattr(_C, n, spy(n))
    try:
        with torch.no_grad():
            out = GaussianRasterizer(settings, contrib_stats=contrib, contrib_pixel_weight=opts.pop("m", None), **opts)(
                means3D=inp["means3D"], means2D=torch.zeros_like(inp["means3D"]), opacities=inp["opacities"], shs=inp["shs"],
                scales=inp["scales"], rotations=inp["rotations"])
    finally:
        for n in names:
            setattr(_C, n, orig[n])
    torch.cuda.synchronize()
    return out, cap["r"]


@pytest.mark.parametrize("opts", [{}, {"antialiasing": True}, {"depth_alpha": "depth"}], ids=["default", "antialiasing", "depth"])
def test_through_the_module(opts):
    """Assertion 7: GaussianRasterizer(contrib_stats=...) under no_grad fills the tensors with what _C.gaussian_contributions gives on
    the captured state -- checked against the walk over that run's records -- and leaves colour and radii bit-identical."""
    _need_gpu()
    c = _case("B")
    P, W, H, cam = c["P"], c["W"], c["H"], c["cam"]
    m = c["m"].to(_dev())
    s = _stats(P)
    out, r = _module_run(c, s, m=m.reshape(1, H, W), **opts)
    plain, _ = _module_run(c, None, **opts)
    assert len(out) == len(plain) == (4 if "depth_alpha" in opts else 2)
    for a, b in zip(out, plain):
        assert torch.equal(a, b)
    got = tuple(t.cpu().numpy() for t in s)
    direct = _contrib(r, P, cam, m)
    for x, y in zip(_bits(got), _bits(direct)):
        assert np.array_equal(x, y)
    st = util.unpack_state(dict(R=r[0], geom=r[3], binning=r[4], img=r[5]), P, W, H)
    _check_against(ref_walk(st, W, H, c["m"].numpy()), got, W * H, f"contrib B module {opts}")
    if opts.get("antialiasing"):   # the compensated opacity is what blends: the weights differ from the default path's
        assert not np.array_equal(got[0], _contrib(c["r"], P, cam, m)[0])


def test_render_on_the_leaf_path_agrees_with_the_module_path():
    """Assertion 7, last item.  On either path render() must fill the tensors with what _C.gaussian_contributions gives on the state
    of that run's forward, bit for bit (the leaf path's state is captured at fused_params._leaf_forward).  Between the two paths only
    a sanity check is possible: the leaf path activates inside the kernel, so its records may differ from the module path's in the
    last bit and a threshold decision may flip; each flip moves one Gaussian's count by 1 and its sum by at most the w of that pair
    (alpha ~ 1 / 255 or T ~ 1e-4: below 0.004).  Bars there: counts within 2 and equal for 99 % of the Gaussians, sums within 1e-4
    relative + 0.01, maxima within 1e-4 relative + 0.004; the image-wide total within 1e-4."""
    _need_gpu()
    import fused_params
    import gsr_model
    from diff_gaussian_rasterization import _C
    from gaussian_renderer import render
    c = _case("B")
    P, cam, scene, dev = c["P"], c["cam"], c["scene"], _dev()
    camd = cam._replace(world_view_transform=cam.world_view_transform.to(dev), full_proj_transform=cam.full_proj_transform.to(dev),
                        camera_center=cam.camera_center.to(dev))
    cap = {}
    spied = {(fused_params, "_leaf_forward"): slice(3, 6), (_C, "rasterize_gaussians"): slice(3, 6)}   # -> (geom, binning, img); R first
    orig = {k: getattr(*k) for k in spied}

    def spy(k):
        def f(*a, **kw):
            out = orig[k](*a, **kw)
            cap["r"] = (out[0], None, None, *out[spied[k]])
            return out
        return f
    res = {}
    for k in spied:
        setattr(*k, spy(k))
    try:
        for fused in (False, True):
            pc = gsr_model.GaussianParams.from_activated(scene.means3D, scene.shs, scene.scales, scene.rotations, scene.opacities, max_sh_degree=D, active_sh_degree=D, device=dev)
            s = _stats(P)
            cap.clear()
            with torch.no_grad():
                out = render(camd, pc, gsr_model.pipeline_params(fused_activations=fused), scene.bg.to(dev), contrib_stats=s)
            assert set(out) == {"render", "viewspace_points", "visibility_filter", "radii"}
            torch.cuda.synchronize()
            got = tuple(t.cpu().numpy() for t in s)
            for x, y in zip(_bits(got), _bits(_contrib(cap["r"], P, cam))):
                assert np.array_equal(x, y), f"fused_activations={fused}"
            res[fused] = tuple(x.astype(np.float64) for x in got)
    finally:
        for k in spied:
            setattr(*k, orig[k])
    (s0, x0, n0), (s1, x1, n1) = res[False], res[True]
    assert n0.sum() > 0 and bool((np.abs(n0 - n1) <= 2).all()) and float((n0 == n1).mean()) >= 0.99
    assert bool((np.abs(s0 - s1) <= 1e-4 * s0 + 0.01).all()) and bool((np.abs(x0 - x1) <= 1e-4 * x0 + 0.004).all())
    assert abs(s0.sum() - s1.sum()) <= 1e-4 * s0.sum()


def test_nothing_to_do():
    """Assertion 8 (C): P = 0, one Gaussian, and a scene behind the camera (num_rendered = 0): no error, and only what blended is written."""
    _need_gpu()
    from diff_gaussian_rasterization import _C
    cam = gsr_scene.make_camera(33, 17)
    empty = gsr_scene.make_scene(0, -3.0, sh_degree=D, seed=1)
    r, _ = _forward(empty, cam)
    assert r[0] == 0
    got = _contrib(r, 0, cam)
    assert all(x.size == 0 for x in got)
    scene = gsr_scene.make_scene(50, -3.0, sh_degree=D, seed=2)
    behind = scene._replace(means3D=scene.means3D - torch.tensor([0.0, 0.0, 20.0]))   # the camera sits at z = -4 and looks down +z
    r, _ = _forward(behind, cam)
    assert r[0] == 0
    got = _contrib(r, 50, cam, fill=(-3.0, -1.0, -5))
    assert bool((got[0] == -3.0).all()) and bool((got[1] == -1.0).all()) and bool((got[2] == -5).all())
    one = gsr_scene.make_scene(1, -1.5, sh_degree=D, seed=4)
    one = one._replace(means3D=torch.zeros(1, 3), opacities=torch.full((1, 1), 0.8))
    r, _ = _forward(one, cam)
    assert r[0] > 0
    st = util.unpack_state(dict(R=r[0], geom=r[3], binning=r[4], img=r[5]), 1, 33, 17)
    got = _contrib(r, 1, cam)
    _check_against(ref_walk(st, 33, 17), got, 33 * 17, "contrib one Gaussian", guard=False)
    assert got[2][0] > 0 and abs(float(got[0][0]) - float((1.0 - st["final_T"].astype(np.float64)).sum())) <= 1e-5 * float(got[0][0])
    # only pixel_count asked for
    n_only = torch.zeros(1, dtype=torch.int32, device=_dev())
    _C.gaussian_contributions(r[3], r[4], r[5], r[0], 1, 33, 17, (None, None, n_only))
    assert int(n_only.cpu()[0]) == int(got[2][0])
