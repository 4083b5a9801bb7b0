"""GPU: the 4D Gaussian time slice and the harmonic colour coefficients (include/gsr_slice4d.h, fused_slice4d.py) against
tests/torch_slice4d.py in float64, through the raw entry points with guard rows behind every output, and through render(time=).

P in {1, 63, 64, 65, 255, 256, 257, 1000}: a lone lane, waves that are not full, one below / at / one above the workgroup of 256 (the
harmonic kernels own 64 rows per workgroup, so 63 / 64 / 65 are their seam), several workgroups with a remainder.  Rows whose temporal
marginal lies within 2^-40 relative of the cutoff are skipped (tests/test_slice4d_cpu.py caps them at 1 %; there are none).

Bars, derived and not tuned -- one rounding to float32 plus double-precision error under the cancellation of the formula:
    means3D      2^-24 |ref| + 2^-40 (|xyz| + |velocity D|)
    cov3D        2^-24 |ref| + 2^-40 (|Sigma_11,ij| + |u_i u_j / Sigma_tt|)
    opacities, velocity   (2^-24 + 2^-40) |ref|;  masked rows exactly +0, the mask the reference's
    leaf gradients, per element   2^-24 |ref| + 2^-40 (the row's largest sum of the moduli of the terms the gradient is formed from,
                 torch_slice4d.slice4d_grads(absolute=True): the first form the issue names, not the fallback);  masked rows exactly +0
    shs          (N + 2) 2^-24 sum_n |c_n f_n|;   dfeatures_t 2^-24 |ref| (one rounding) + 2^-24 |g| 2^-24 (the coefficient's own rounding
                 sits in the reference);   dt 2^-24 |ref| + 2^-40 sum |terms|
Measured on the MI355X (this file, printed by the tests; error / bar, the largest over all P):
    forward      means3D 0.991, cov3D 0.991, opacities 0.977, velocity 0.983 (one rounding to float32 is 1.0 of these bars);
                 the stock float32 sequence on the same inputs: means3D 387, cov3D 5857, opacities 24.5, velocity 3576
    backward     dL/dxyz 0 (a copy), dL/dt 0.990, dL/dscaling 0.995, dL/dscaling_t 0.968, dL/drotation 0.992, dL/drotation_r 0.988,
                 dL/dopacity 0.956
    harmonics    shs 0.466, dfeatures_t 1.000, dt 0.977
    render       leaf gradients 0.996 at most; the static limit differs from the static render by 8.05e-6 at most, radii equal
"""
import math

import pytest
import torch

import torch_slice4d as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
A, B = 2.0 ** -24, 2.0 ** -40
GUARD = 64          # canary rows behind every output
CANARY = -777.25
OUT_COLS = (3, 6, 1, 3)
OUT_NAMES = ("means3D", "cov3D", "opacities", "velocity")
_cache = {}


def _padded(P, cols):
    return torch.full((P + GUARD, cols), CANARY, dtype=torch.float32, device=DEV)


def _intact(buf, P):
    return bool((buf[P:] == CANARY).all())


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _case(P):
    """-> leaves and incoming gradients (CPU and device), the float64 slice, its bars; computed once, never written to"""
    if P not in _cache:
        lv, inc = ref.make_scene(P, seed=P), ref.make_incoming(P, seed=P)
        sl = ref.slice4d(lv)
        _cache[P] = dict(lv=lv, inc=inc, sl=sl, bars=ref.forward_bars(sl, lv), keep=~ref.ambiguous(sl), dlv=[lv[k].to(DEV) for k in ref.LEAVES],
                         dinc=[g.to(DEV) for g in inc], grads={})
    return _cache[P]


def _grads(case, present=(True,) * 4):
    """-> (reference gradients from autograd, per-element bars) with the incoming gradients of `present`; cached"""
    if present not in case["grads"]:
        inc = tuple(g if p else None for g, p in zip(case["inc"], present))
        auto = ref.autograd_grads(case["lv"], inc)
        scale = ref.slice4d_grads(case["lv"], inc, absolute=True)
        bars = {k: A * auto[k].abs() + B * scale[k].amax(dim=1, keepdim=True) for k in ref.LEAVES}
        case["grads"][present] = (auto, bars)
    return case["grads"][present]


def _forward_raw(case, P, outs=(True,) * 4):
    import fused_slice4d as fs
    bufs = [_padded(P, c) if on else None for c, on in zip(OUT_COLS, outs)]
    fs._run("gsr_slice4d_forward", P, *(x.data_ptr() for x in case["dlv"]), ref.TIME, 1.0, ref.CUTOFF, *(_ptr(b) for b in bufs), _stream())
    torch.cuda.synchronize()
    assert all(b is None or _intact(b, P) for b in bufs)
    return [None if b is None else b[:P] for b in bufs]


def _backward_raw(case, P, present=(True,) * 4, outs=(True,) * 7):
    import fused_slice4d as fs
    bufs = [_padded(P, ref.COLS[k]) if on else None for k, on in zip(ref.LEAVES, outs)]
    gin = [g if p else None for g, p in zip(case["dinc"], present)]
    fs._run("gsr_slice4d_backward", P, *(x.data_ptr() for x in case["dlv"]), ref.TIME, 1.0, ref.CUTOFF, *(_ptr(g) for g in gin),
            *(_ptr(b) for b in bufs), _stream())
    torch.cuda.synchronize()
    assert all(b is None or _intact(b, P) for b in bufs)
    return [None if b is None else b[:P] for b in bufs]


def _worst(got, want, bar, rows=None):
    r = (got.double().cpu() - want).abs() / bar.clamp(min=1e-300)
    r = torch.where((bar == 0) & (got.double().cpu() == want), torch.zeros_like(r), r)
    if rows is not None:
        r = r[rows]
    return float(r.max()) if r.numel() else 0.0


def _is_plus_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


@pytest.mark.parametrize("P", ref.GPU_SIZES)
def test_forward_matches_the_float64_reference(P):
    import fused_slice4d as fs
    case = _case(P)
    sl, keep = case["sl"], case["keep"]
    before = [x.clone() for x in case["dlv"]]
    outs = _forward_raw(case, P)
    assert all(torch.equal(a, b) for a, b in zip(before, case["dlv"]))   # the inputs keep their bits
    assert int((~keep).sum()) <= P // 100
    masked = (outs[2][:, 0] == 0).cpu()
    assert torch.equal(masked[keep], sl.mask[keep])
    assert _is_plus_zero(outs[2][masked.to(DEV)])
    s32 = ref.slice4d(case["lv"], dtype=torch.float32)
    live = keep & ~sl.mask
    for name, got in zip(OUT_NAMES, outs):
        rows = keep if name != "opacities" else live
        worst = _worst(got, getattr(sl, name), case["bars"][name], rows)
        stock = _worst(getattr(s32, name), getattr(sl, name), case["bars"][name], live)
        print(f"P = {P}: {name}: largest error / bar {worst:.3f}; the stock float32 sequence on the same inputs {stock:.1f}")
        assert worst <= 1.0, (name, worst)
    # the autograd surface: the same bits, with and without the velocity; two runs, the same bits
    for _ in range(2):
        again = fs.slice_at(*case["dlv"], ref.TIME, velocity=True)
        assert all(torch.equal(a, b) and a.dtype == torch.float32 for a, b in zip(again, outs))
    three = fs.slice_at(*case["dlv"], ref.TIME)
    assert len(three) == 3 and all(torch.equal(a, b) for a, b in zip(three, outs))
    assert torch.equal(fs.visible_at(outs[2]), ~masked.to(DEV))
    # each output in turn is left out
    for drop in range(4):
        some = _forward_raw(case, P, tuple(n != drop for n in range(4)))
        assert some[drop] is None and all(torch.equal(a, b) for n, (a, b) in enumerate(zip(some, outs)) if n != drop)
    # strided inputs
    strided = []
    for x in case["dlv"]:
        wide = torch.zeros(P, 2 * x.shape[1], device=DEV)[:, ::2]
        wide.copy_(x)
        strided.append(wide)
    assert all(torch.equal(a, b) for a, b in zip(fs.slice_at(*strided, ref.TIME, velocity=True), outs))
    # other scalars: the modifier and a cutoff of 0 (no row masked)
    other = fs.slice_at(*case["dlv"], ref.TIME + 0.1, scaling_modifier=0.7, cutoff=0.0)
    sl2 = ref.slice4d(case["lv"], time=ref.TIME + 0.1, scaling_modifier=0.7, cutoff=0.0)
    bars2 = ref.forward_bars(sl2, case["lv"], time=ref.TIME + 0.1)
    tiny = (sl2.opacities.abs() < 1e-37)[:, 0]   # float32 underflow
    for name, got in zip(OUT_NAMES, other):
        assert _worst(got, getattr(sl2, name), bars2[name], ~tiny if name == "opacities" else None) <= 1.0, name


@pytest.mark.parametrize("P", ref.GPU_SIZES)
def test_backward_matches_autograd_through_the_reference(P):
    import fused_slice4d as fs
    case = _case(P)
    sl, keep = case["sl"], case["keep"]
    auto, bars = _grads(case)
    got = _backward_raw(case, P)
    mask = sl.mask & keep
    for k, g in zip(ref.LEAVES, got):
        worst = _worst(g, auto[k], bars[k], keep)
        print(f"P = {P}: dL/d{k}: largest error / bar {worst:.3f}")
        assert worst <= 1.0, (k, worst)
        assert _is_plus_zero(g[mask.to(DEV)]), k
    assert all(torch.equal(a, b) for a, b in zip(_backward_raw(case, P), got))   # two runs, the same bits
    # each incoming gradient in turn is absent
    for drop in range(4):
        present = tuple(n != drop for n in range(4))
        auto_d, bars_d = _grads(case, present)
        for k, g in zip(ref.LEAVES, _backward_raw(case, P, present)):
            assert _worst(g, auto_d[k], bars_d[k], keep) <= 1.0, (drop, k)
            assert _is_plus_zero(g[mask.to(DEV)])
    # each output in turn is left out: the others keep their bits
    for drop in range(7):
        some = _backward_raw(case, P, outs=tuple(n != drop for n in range(7)))
        assert some[drop] is None and all(torch.equal(a, b) for n, (a, b) in enumerate(zip(some, got)) if n != drop)
    # the autograd surface, contiguous and strided leaves: the same bits at the leaves
    leaves = [x.clone().requires_grad_(True) for x in case["dlv"]]
    torch.autograd.backward(fs.slice_at(*leaves, ref.TIME, velocity=True), case["dinc"])
    assert all(torch.equal(x.grad, g) for x, g in zip(leaves, got))
    wide = []
    for x in case["dlv"]:   # every leaf is every other column of a tensor twice as wide
        base = torch.zeros(P, 2 * x.shape[1], device=DEV)
        base[:, ::2] = x
        wide.append(base.requires_grad_(True))
    torch.autograd.backward(fs.slice_at(*(b[:, ::2] for b in wide), ref.TIME, velocity=True), case["dinc"])
    assert all(torch.equal(b.grad[:, ::2], g) and bool((b.grad[:, 1::2] == 0).all()) for b, g in zip(wide, got))
    # only some leaves need a gradient, only some outputs are used
    leaves = [x.detach().clone().requires_grad_(k in ("t", "rotation_r")) for k, x in zip(ref.LEAVES, case["dlv"])]
    means, cov, opac = fs.slice_at(*leaves, ref.TIME)
    (cov * case["dinc"][1]).sum().backward()
    auto_c, bars_c = _grads(case, (False, True, False, False))
    for k, x in zip(ref.LEAVES, leaves):
        if k in ("t", "rotation_r"):
            assert _worst(x.grad, auto_c[k], bars_c[k], keep) <= 1.0, k
        else:
            assert x.grad is None


@pytest.mark.parametrize("P", ref.GPU_SIZES)
@pytest.mark.parametrize("M", (1, 4, 16))
@pytest.mark.parametrize("N", (0, 1, 3))
def test_harmonic_features_match_the_float64_reference(N, M, P):
    import fused_slice4d as fs
    case = _case(P)
    f, g = ref.make_features(P, N, M, seed=P)
    t = case["lv"]["t"]
    period = 0.8
    df, dg, dt_ = f.to(DEV), g.to(DEV), case["dlv"][1]
    shs = _padded(P * M, 3)
    d_f, d_t = _padded(P * (N + 1) * M, 3), _padded(P, 1)
    fs._run("gsr_harmonic_features", P, N, M, df.data_ptr(), dt_.data_ptr(), ref.TIME, period, shs.data_ptr(), _stream())
    fs._run("gsr_harmonic_features_backward", P, N, M, df.data_ptr(), dt_.data_ptr(), ref.TIME, period, dg.data_ptr(), d_f.data_ptr(), d_t.data_ptr(),
            _stream())
    torch.cuda.synchronize()
    assert _intact(shs, P * M) and _intact(d_f, P * (N + 1) * M) and _intact(d_t, P)
    shs, d_f, d_t = shs[:P * M].view(P, M, 3), d_f[:P * (N + 1) * M].view(P, N + 1, M, 3), d_t[:P]
    want, scale = ref.harmonic(f, t, ref.TIME, period)
    r_f, r_t, terms = ref.harmonic_grads(f, t, ref.TIME, period, g)
    w = (_worst(shs, want, (N + 2) * A * scale), _worst(d_f, r_f, A * r_f.abs()), _worst(d_t, r_t, A * r_t.abs() + B * terms))
    print(f"N = {N}, M = {M}, P = {P}: error / bar: shs {w[0]:.3f}, dfeatures_t {w[1]:.3f}, dt {w[2]:.3f}")
    assert max(w) <= 1.0, w
    if N == 0:
        assert torch.equal(shs, df[:, 0]) and torch.equal(d_f[:, 0], dg) and _is_plus_zero(d_t)
    # the autograd surface, twice: the same bits; strided inputs; one gradient alone
    for strided in (False, True):
        if strided:
            wide = torch.zeros(P, N + 1, M, 6, device=DEV)[..., ::2]
            wide.copy_(df)
            a = wide.requires_grad_(True)
        else:
            a = df.clone().requires_grad_(True)
        b = dt_.clone().requires_grad_(True)
        out = fs.harmonic_features(a, b, ref.TIME, period)
        out.backward(dg)
        assert torch.equal(out, shs) and torch.equal(a.grad, d_f) and torch.equal(b.grad, d_t)
    b = dt_.clone().requires_grad_(True)
    fs.harmonic_features(df, b, ref.TIME, period).backward(dg)
    assert torch.equal(b.grad, d_t)
    only_t = _padded(P, 1)
    fs._run("gsr_harmonic_features_backward", P, N, M, df.data_ptr(), dt_.data_ptr(), ref.TIME, period, dg.data_ptr(), None, only_t.data_ptr(), _stream())
    only_f = _padded(P * (N + 1) * M, 3)
    fs._run("gsr_harmonic_features_backward", P, N, M, df.data_ptr(), dt_.data_ptr(), ref.TIME, period, dg.data_ptr(), only_f.data_ptr(), None, _stream())
    torch.cuda.synchronize()
    assert _intact(only_t, P) and torch.equal(only_t[:P], d_t) and _intact(only_f, P * (N + 1) * M)
    assert torch.equal(only_f[:P * (N + 1) * M].view(P, N + 1, M, 3), d_f)


def test_harmonic_features_without_alignment_take_the_narrow_path():
    """3 M a multiple of four, but pointers at an odd multiple of four bytes: the 4-byte kernels, the same bits"""
    import fused_slice4d as fs
    P, N, M = 257, 2, 4
    case = _case(P)
    f, g = ref.make_features(P, N, M, seed=5)
    df, dg, dt_ = f.to(DEV), g.to(DEV), case["dlv"][1]
    a = df.clone().requires_grad_(True)
    want = fs.harmonic_features(a, dt_, ref.TIME, 0.8)
    want.backward(dg)
    shifted_f = torch.zeros(df.numel() + 1, device=DEV)
    shifted_f[1:] = df.flatten()
    shifted_g = torch.zeros(dg.numel() + 1, device=DEV)
    shifted_g[1:] = dg.flatten()
    shs, d_f = torch.full((P * M * 3 + 1 + GUARD,), CANARY, device=DEV), torch.full((df.numel() + 1 + GUARD,), CANARY, device=DEV)
    fs._run("gsr_harmonic_features", P, N, M, shifted_f.data_ptr() + 4, dt_.data_ptr(), ref.TIME, 0.8, shs.data_ptr() + 4, _stream())
    fs._run("gsr_harmonic_features_backward", P, N, M, shifted_f.data_ptr() + 4, dt_.data_ptr(), ref.TIME, 0.8, shifted_g.data_ptr() + 4,
            d_f.data_ptr() + 4, None, _stream())
    torch.cuda.synchronize()
    assert torch.equal(shs[1:1 + P * M * 3], want.detach().flatten()) and bool((shs[1 + P * M * 3:] == CANARY).all()) and float(shs[0]) == CANARY
    assert torch.equal(d_f[1:1 + df.numel()], a.grad.flatten()) and bool((d_f[1 + df.numel():] == CANARY).all()) and float(d_f[0]) == CANARY


def test_slice_without_quaternion_alignment_gives_the_same_bits():
    """quaternions and their gradients at an odd multiple of four bytes: four 4-byte accesses instead of one 16-byte access"""
    import fused_slice4d as fs
    P = 257
    case = _case(P)
    want_f, want_b = _forward_raw(case, P), _backward_raw(case, P)

    def shifted(x):
        buf = torch.full((x.numel() + 1 + GUARD,), CANARY, device=DEV)
        buf[1:1 + x.numel()] = x.flatten()
        return buf

    lv = list(case["dlv"])
    quats = [shifted(lv[4]), shifted(lv[5])]
    ptrs = [x.data_ptr() for x in lv]
    ptrs[4], ptrs[5] = quats[0].data_ptr() + 4, quats[1].data_ptr() + 4
    outs = [_padded(P, c) for c in OUT_COLS]
    fs._run("gsr_slice4d_forward", P, *ptrs, ref.TIME, 1.0, ref.CUTOFF, *(b.data_ptr() for b in outs), _stream())
    grads = [_padded(P, ref.COLS[k]) for k in ref.LEAVES]
    dq = [shifted(torch.zeros(P, 4, device=DEV)) for _ in range(2)]
    gptrs = [b.data_ptr() for b in grads]
    gptrs[4], gptrs[5] = dq[0].data_ptr() + 4, dq[1].data_ptr() + 4
    fs._run("gsr_slice4d_backward", P, *ptrs, ref.TIME, 1.0, ref.CUTOFF, *(g.data_ptr() for g in case["dinc"]), *gptrs, _stream())
    torch.cuda.synchronize()
    assert all(_intact(b, P) and torch.equal(b[:P], w) for b, w in zip(outs, want_f))
    for k, (b, w) in enumerate(zip(grads, want_b)):
        if k in (4, 5):
            got = dq[k - 4]
            assert torch.equal(got[1:1 + 4 * P].view(P, 4), w) and float(got[0]) == CANARY and bool((got[1 + 4 * P:] == CANARY).all())
            assert bool((b == CANARY).all())
        else:
            assert _intact(b, P) and torch.equal(b[:P], w)


# ---- render(time=) ----
W, H, PR = 200, 120, 2000
TAU = 0.37


def _scene():
    if "render" not in _cache:
        import gsr_scene
        scene = gsr_scene.make_scene(PR, -3.0, sh_degree=3, seed=3)
        cam = gsr_scene.make_camera(W, H)
        camd = cam._replace(world_view_transform=cam.world_view_transform.to(DEV), full_proj_transform=cam.full_proj_transform.to(DEV),
                            camera_center=cam.camera_center.to(DEV))
        g = torch.Generator().manual_seed(21)
        extra = dict(t=(TAU - 0.3 * torch.randn(PR, 1, generator=g)), scaling_t=-2.0 + 0.7 * torch.randn(PR, 1, generator=g),
                     rotation_r=scene.rotations + 0.3 * torch.randn(PR, 4, generator=g),
                     features_t=torch.cat((scene.shs[:, None], 0.3 * torch.randn(PR, 2, 16, 3, generator=g)), dim=1))
        dpix = torch.randn(3, H, W, generator=g).to(DEV)
        _cache["render"] = (scene, camd, extra, dpix)
    return _cache["render"]


def _model4d(harmonics, static=False):
    import gsr_model
    scene, camd, extra, dpix = _scene()
    pc = gsr_model.GaussianParams.from_activated(scene.means3D, scene.shs, scene.scales, scene.rotations, scene.opacities, device=DEV,
                                                 active_sh_degree=3)
    leaf = lambda t: t.to(DEV).clone().requires_grad_(True)
    if static:
        pc._t, pc._scaling_t, pc._rotation_r = leaf(torch.full((PR, 1), TAU)), leaf(torch.full((PR, 1), 5.0)), leaf(scene.rotations)
    else:
        pc._t, pc._scaling_t, pc._rotation_r = leaf(extra["t"]), leaf(extra["scaling_t"]), leaf(extra["rotation_r"])
    if harmonics:
        pc._features_t, pc.time_period = leaf(extra["features_t"]), 0.8
    return pc


def _leaves(pc):
    return (pc._xyz, pc._t, pc._scaling, pc._scaling_t, pc._rotation, pc._rotation_r, pc._opacity)


@pytest.mark.parametrize("harmonics", (False, True))
def test_render_at_a_time_is_the_rasterizer_fed_the_slice(harmonics):
    import fused_slice4d as fs
    import gaussian_renderer
    import gsr_model
    from diff_gaussian_rasterization import GaussianRasterizer
    scene, camd, extra, dpix = _scene()
    bg = scene.bg.to(DEV)
    pipe = gsr_model.pipeline_params()
    pc = _model4d(harmonics)
    out = gaussian_renderer.render(camd, pc, pipe, bg, time=TAU, depth_alpha="depth")
    (out["render"] * dpix).sum().backward()

    # by hand: the module's own outputs into the rasterizer, the sliced tensors keeping their gradients
    pc2 = _model4d(harmonics)
    means, cov, opac = fs.slice_at(*_leaves(pc2), TAU)
    shs = fs.harmonic_features(pc2._features_t, pc2._t, TAU, 0.8) if harmonics else pc2.get_features
    for x in (means, cov, opac, shs):
        x.retain_grad()
    means2D = torch.zeros_like(means, requires_grad=True)
    settings = gaussian_renderer._settings_for(camd, pc2, pipe, bg, 1.0)
    direct = GaussianRasterizer(raster_settings=settings, depth_alpha="depth")(
        means3D=means, means2D=means2D, opacities=opac, shs=shs, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=cov)
    assert torch.equal(out["render"], direct[0]) and torch.equal(out["radii"], direct[1])
    assert torch.equal(out["depth"], direct[2]) and torch.equal(out["alpha"], direct[3])
    assert int((direct[1] > 0).sum()) > 200
    (direct[0] * dpix).sum().backward()
    assert all(torch.equal(a.grad, b.grad) for a, b in zip(_leaves(pc), _leaves(pc2)))
    assert torch.equal(out["viewspace_points"].grad, means2D.grad) and out["viewspace_points"].shape == (PR, 3)
    if harmonics:
        assert torch.equal(pc._features_t.grad, pc2._features_t.grad) and float(pc._features_t.grad.abs().max()) > 0
    else:
        assert torch.equal(pc._features_dc.grad, pc2._features_dc.grad)

    # the visibility filter excludes masked rows; radii are not touched
    lv = {k: x.detach().cpu() for k, x in zip(ref.LEAVES, _leaves(pc2))}
    sl = ref.slice4d(lv, time=TAU)
    keep = ~ref.ambiguous(sl)
    vis = out["visibility_filter"].cpu()
    assert vis.dtype == torch.bool and not bool(vis[sl.mask & keep].any())
    assert torch.equal(vis, (out["radii"] > 0).cpu() & (opac.detach()[:, 0] > 0).cpu())
    assert int(((out["radii"] > 0).cpu() & sl.mask).sum()) > 0 and int(vis.sum()) > 100

    # the leaf gradients against the float64 chain applied to the rasterizer's own dL/dmeans3D, dL/dcov3D, dL/dopacities (the time
    # leaf also receives the harmonics' share, taken from the float64 formula of the same dL/dshs)
    inc = (means.grad.cpu(), cov.grad.cpu(), opac.grad.cpu(), None)
    auto = ref.autograd_grads(lv, inc, time=TAU)
    scale = ref.slice4d_grads(lv, inc, time=TAU, absolute=True)
    extra_t = extra_terms = 0.0
    if harmonics:
        _, extra_t, extra_terms = ref.harmonic_grads(pc2._features_t.detach().cpu(), lv["t"], TAU, 0.8, shs.grad.cpu())
    for k, x in zip(ref.LEAVES, _leaves(pc)):
        want = auto[k] + (extra_t if k == "t" else 0.0)
        bar = A * want.abs() + B * (scale[k] + (extra_terms if k == "t" else 0.0)).amax(dim=1, keepdim=True)
        if k == "t" and harmonics:   # two float32 results are added by autograd: one more rounding of each
            bar = bar + A * (auto[k].abs() + extra_t.abs())
        worst = _worst(x.grad, want, bar, keep)
        print(f"harmonics = {harmonics}: dL/d{k}: largest error / bar {worst:.3f}")
        assert worst <= 1.0, (k, worst)
        assert float(x.grad.abs().max()) > 0


def test_render_of_the_static_limit_equals_the_static_render():
    import gaussian_renderer
    import gsr_model
    scene, camd, extra, dpix = _scene()
    bg = scene.bg.to(DEV)
    pipe = gsr_model.pipeline_params()
    pc = _model4d(False, static=True)
    out = gaussian_renderer.render(camd, pc, pipe, bg, time=TAU)
    static = gaussian_renderer.render(camd, pc, pipe, bg)
    err = float((out["render"] - static["render"]).detach().abs().max())
    print(f"static limit: image max abs difference {err:.2e}; radii equal: {bool(torch.equal(out['radii'], static['radii']))}")
    assert err <= 1e-5
    assert bool(out["visibility_filter"].any())


def test_render_without_a_time_is_the_call_without_the_keyword():
    import gaussian_renderer
    import gsr_model
    scene, camd, extra, dpix = _scene()
    bg = scene.bg.to(DEV)
    for fused in (False, True):
        pipe = gsr_model.pipeline_params(fused_activations=fused)
        a, b = _model4d(True), _model4d(True)
        plain = gaussian_renderer.render(camd, a, pipe, bg)
        none = gaussian_renderer.render(camd, b, pipe, bg, time=None)
        assert torch.equal(plain["render"], none["render"]) and torch.equal(plain["radii"], none["radii"])
        assert torch.equal(plain["visibility_filter"], none["visibility_filter"])
        (plain["render"] * dpix).sum().backward()
        (none["render"] * dpix).sum().backward()
        for x, y in zip(a.parameters(), b.parameters()):
            assert torch.equal(x.grad, y.grad)
        assert a._t.grad is None and b._t.grad is None
