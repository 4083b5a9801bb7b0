"""GPU: Mip-Splatting's 3D smoothing filter (include/gsr_filter3d.h, fused_filter3d.py) against tests/torch_filter3d.py in float64.

Sweep, (P, C) of torch_filter3d.SWEEP_CASES (a lone lane, waves that are not full, one below / at / one above the workgroup of 256,
several workgroups with a remainder; the cameras are not chunked, so C has no seam), both per_camera settings.  Rows whose decision
lies inside the fp32 error of its own inputs are skipped (tests/test_filter3d_cpu.py caps them at 1 % and shows that none of them
can set the fill value); every other row is within
    sqrt(0.2) 16 * 2^-24 (sum_k |R_2k x_k| + |t_2|) / f  +  4 * 2^-24 ref
of the reference: the three-term dot product with its translation (three roundings as an fma chain, 16 allowed), carried through
1 / f (f_max, or the winning camera's fx with per_camera); then one division, one product and the rounded constant (2.5 * 2^-24
relative in all, 4 allowed).  Derived, not measured.  Rows valid nowhere carry the bits of the row with the largest valid distance.
Activations, P in {1, 63, 64, 65, 257, 1000}: outputs and dL/dlogit within 16 * 2^-24 relative, dL/dlog-scale within
16 * 2^-24 (|term1| + |term2|) of the reference's two terms (they may cancel).  The kernels evaluate in double and round once, so the
achieved figure is the rounding to float32 and what the device's double exp and sqrt leave.
Measured on the MI355X (this file, printed by the tests):
    sweep        largest error / bar over all cases: 0.137, with either per_camera setting
    activations  opacities 0.97, scales 0.95, dL/dlogit 0.97, dL/dlog-scale 0.99 (in units of 2^-24, P = 1000: one rounding);
                 the stock fp32 sequence on the same inputs: opacities 4.86, scales 2.41
    reset        all 632 rows at or above the cap 0 ulp; baked leaves: all 4264 values 0 ulp
"""
import pytest
import torch

import torch_filter3d as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
GUARD = 64          # canary rows behind every output
CANARY = -777.25
_cache = {}


def _padded(P, cols):
    return torch.full((P + GUARD, cols), CANARY, dtype=torch.float32, device=DEV)


def _intact(buf, P):
    return bool((buf[P:] == CANARY).all())


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _sweep_case(P, C):
    """-> xyz and packed records on the device, and the float64 references of both settings; computed once, never written to"""
    import fused_filter3d as ff
    if (P, C) not in _cache:
        xyz, cams = ref.sweep_scene(P, C)
        rec = ff.pack_cameras(cams, "cpu")
        _cache[(P, C)] = (xyz.to(DEV), rec.to(DEV), {pc: ref.sweep(xyz, rec, pc) for pc in (False, True)}, cams)
    return _cache[(P, C)]


@pytest.mark.parametrize("per_camera", (False, True))
@pytest.mark.parametrize("P,C", ref.SWEEP_CASES)
def test_sweep_matches_the_float64_reference(P, C, per_camera):
    import fused_filter3d as ff
    xyz, rec, refs, cams = _sweep_case(P, C)
    r = refs[per_camera]
    # the entry point itself, with guard rows behind the output
    lib = ff._lib()
    out = _padded(P, 1)
    scratch = torch.empty(lib.gsr_filter3d_scratch_bytes(P), dtype=torch.uint8, device=DEV)
    ff._run("gsr_filter3d_compute", P, C, xyz.data_ptr(), rec.data_ptr(), int(per_camera), out.data_ptr(), scratch.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert _intact(out, P)
    got = out[:P]
    again = ff.compute_filter_3d(xyz, rec, per_camera)
    assert again.shape == (P, 1) and again.dtype == torch.float32 and torch.equal(again, got)           # two runs, the same bits
    assert torch.equal(ff.compute_filter_3d(xyz, cams, per_camera), got)                                # a list is packed to the same records
    perm = torch.randperm(C, generator=torch.Generator().manual_seed(C)).to(DEV)
    assert torch.equal(ff.compute_filter_3d(xyz, rec[perm], per_camera), got)                           # any order of the cameras
    assert torch.equal(ff.compute_filter_3d(xyz, rec.flip(0), per_camera), got)
    strided = torch.zeros(P, 6, device=DEV)[:, ::2]
    strided.copy_(xyz)
    assert not strided.is_contiguous() or P == 1
    assert torch.equal(ff.compute_filter_3d(strided.requires_grad_(True), rec, per_camera), got)

    g = got[:, 0].double().cpu()
    keep = ~r.ambiguous
    assert int((~keep).sum()) <= P // 100
    bound = ref.sweep_bound(r)
    err = (g - r.filter).abs()
    worst = float((err[keep] / bound[keep]).max())
    print(f"P = {P}, C = {C}, per_camera = {per_camera}: largest error / bar {worst:.3f} over {int(keep.sum())} rows; {int((~r.seen).sum())} valid nowhere")
    assert bool((err[keep] <= bound[keep]).all())
    lost = keep & ~r.seen
    assert bool((got[:, 0].cpu()[lost].view(torch.int32) == got[r.dmax_row, 0].cpu().view(torch.int32)).all())
    assert not bool(r.ambiguous[r.dmax_row]) and float(err[r.dmax_row]) <= float(bound[r.dmax_row])


@pytest.mark.parametrize("per_camera", (False, True))
def test_sweep_without_a_valid_row_gives_the_sentinel(per_camera):
    import fused_filter3d as ff
    xyz, cams = ref.unseen_scene()
    got = ff.compute_filter_3d(xyz.to(DEV), cams, per_camera)
    assert bool((got == ref.UNSEEN).all()) and ff.UNSEEN == ref.UNSEEN


# ---- activations ----
def _activation_case(P, **kw):
    key = ("act", P, tuple(sorted(kw.items())))
    if key not in _cache:
        opacity, scaling, f = ref.make_leaves(P, seed=P, **kw)
        g = torch.Generator().manual_seed(100 + P)
        g_o, g_s = torch.randn(P, 1, generator=g), torch.randn(P, 3, generator=g)
        _cache[key] = (opacity, scaling, f, g_o, g_s)
    return _cache[key]


def _rel(got, want64):
    return float(((got.double().cpu() - want64).abs() / want64.abs()).max() / U)


def _check_activations(opacity, scaling, f, g_o, g_s, label, floor=None):
    """forward and backward through the entry points with guard rows, against the reference; floor: the modulus under which a value
    that underflows in the reference only has to be that small itself"""
    import fused_filter3d as ff
    P = opacity.shape[0]
    dl, dls, df, dgo, dgs = (t.to(DEV) for t in (opacity, scaling, f, g_o, g_s))
    before = [t.clone() for t in (dl, dls, df, dgo, dgs)]
    o, s, d_o, d_s = _padded(P, 1), _padded(P, 3), _padded(P, 1), _padded(P, 3)
    ff._run("gsr_filter3d_activate", P, dl.data_ptr(), dls.data_ptr(), df.data_ptr(), o.data_ptr(), s.data_ptr(), _stream())
    ff._run("gsr_filter3d_activate_backward", P, dl.data_ptr(), dls.data_ptr(), df.data_ptr(), dgo.data_ptr(), dgs.data_ptr(), d_o.data_ptr(),
            d_s.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert all(_intact(b, P) for b in (o, s, d_o, d_s))
    assert all(torch.equal(a, b) for a, b in zip(before, (dl, dls, df, dgo, dgs)))   # the inputs keep their bits
    o, s, d_o, d_s = o[:P], s[:P], d_o[:P], d_s[:P]
    for t in (o, s, d_o, d_s):
        assert bool(torch.isfinite(t).all())
    r_o, r_s, _ = ref.activations(opacity, scaling, f)
    r_dl, t1, t2 = ref.activation_grads(opacity, scaling, f, g_o, g_s)

    def within(got, want, scale, name):
        err = (got.double().cpu() - want).abs()
        ok = err <= 16 * U * scale
        if floor is not None:
            ok = ok | ((want.abs() < floor) & (got.double().cpu().abs() < floor))
        worst = float((err / scale.clamp(min=1e-300)).max() / U)
        assert bool(ok.all()), (label, name, worst)
        return worst

    figures = {"opacities": within(o, r_o, r_o.abs(), "opacities"), "scales": within(s, r_s, r_s.abs(), "scales"),
               "dL/dlogit": within(d_o, r_dl, r_dl.abs(), "dL/dlogit"), "dL/dlog-scale": within(d_s, t1 + t2, t1.abs() + t2.abs(), "dL/dlog-scale")}
    print(f"{label}: " + ", ".join(f"{k} {v:.2f}" for k, v in figures.items()) + " (units of 2^-24)")
    return dl, dls, df, dgo, dgs, o, s, d_o, d_s


@pytest.mark.parametrize("P", (1, 63, 64, 65, 257, 1000))
def test_activations_match_the_float64_reference(P):
    import fused_filter3d as ff
    opacity, scaling, f, g_o, g_s = _activation_case(P)
    dl, dls, df, dgo, dgs, o, s, d_o, d_s = _check_activations(opacity, scaling, f, g_o, g_s, f"P = {P}")
    # the stock fp32 sequence's own error on the same inputs, for the record
    r_o, r_s, _ = ref.activations(opacity, scaling, f)
    so, ss = ref.stock_activations(opacity, scaling, f, torch.float32)
    print(f"P = {P}: stock fp32 sequence: opacities {_rel(so, r_o):.2f}, scales {_rel(ss, r_s):.2f} (units of 2^-24)")
    # the autograd surface: the same bits, and the gradients arrive at the leaves
    l, ls = dl.clone().requires_grad_(True), dls.clone().requires_grad_(True)
    ao, as_ = ff.filtered_activations(l, ls, df)
    assert torch.equal(ao, o) and torch.equal(as_, s)
    torch.autograd.backward((ao, as_), (dgo, dgs))
    assert torch.equal(l.grad, d_o) and torch.equal(ls.grad, d_s)
    # again: the same bits
    l2, ls2 = dl.clone().requires_grad_(True), dls.clone().requires_grad_(True)
    bo, bs = ff.filtered_activations(l2, ls2, df)
    torch.autograd.backward((bo, bs), (dgo, dgs))
    assert torch.equal(bo, o) and torch.equal(bs, s) and torch.equal(l2.grad, d_o) and torch.equal(ls2.grad, d_s)
    # one output alone
    only = ff.activate(dl, dls, df, want=("scaling",))
    assert list(only) == ["scaling"] and torch.equal(only["scaling"], s)
    assert torch.equal(ff.activate(dl, dls, df, want=("opacity",))["opacity"], o)


@pytest.mark.parametrize("P", (65, 257))
def test_either_upstream_gradient_may_be_absent(P):
    import fused_filter3d as ff
    opacity, scaling, f, g_o, g_s = _activation_case(P)
    dl, dls, df, dgo, dgs = (t.to(DEV) for t in (opacity, scaling, f, g_o, g_s))
    for use_o, use_s in ((True, False), (False, True)):
        l, ls = dl.clone().requires_grad_(True), dls.clone().requires_grad_(True)
        ao, as_ = ff.filtered_activations(l, ls, df)
        loss = (ao * dgo).sum() if use_o else (as_ * dgs).sum()
        loss.backward()
        r_dl, t1, t2 = ref.activation_grads(opacity, scaling, f, g_o if use_o else None, g_s if use_s else None)
        got_l, got_ls = l.grad.double().cpu(), ls.grad.double().cpu()
        assert bool(((got_l - r_dl).abs() <= 16 * U * r_dl.abs()).all())
        assert bool(((got_ls - (t1 + t2)).abs() <= 16 * U * (t1.abs() + t2.abs())).all())
        if not use_o:
            assert bool((l.grad == 0).all())
    # one leaf alone needs a gradient: the other's is not formed
    l = dl.clone().requires_grad_(True)
    ao, as_ = ff.filtered_activations(l, dls, df)
    (ao * dgo).sum().backward()
    assert l.grad is not None and dls.grad is None


def test_extreme_scales_stay_finite():
    ls = torch.tensor([-40.0, -20.0, 20.0]).repeat_interleave(3)[:, None].expand(9, 3).contiguous()
    opacity = torch.tensor([-8.0, 0.0, 8.0]).repeat(3)[:, None].contiguous()
    f = torch.full((9, 1), 1e-3)
    g = torch.Generator().manual_seed(4)
    g_o, g_s = torch.randn(9, 1, generator=g), torch.randn(9, 3, generator=g)
    _check_activations(opacity, ls, f, g_o, g_s, "log-scales -40, -20, +20 at f = 1e-3", floor=1e-37)


# ---- reset ----
def _optimizer(P, seed):
    from fused_params import FusedAdam
    names = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
    opacity, scaling, f = ref.make_leaves(P, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    leaves = [torch.randn(P, 3, generator=g), torch.randn(P, 1, 3, generator=g), torch.randn(P, 2, 3, generator=g), opacity, scaling,
              torch.randn(P, 4, generator=g)]
    params = [torch.nn.Parameter(t.to(DEV)) for t in leaves]
    opt = FusedAdam([{"params": [p], "lr": 1e-3, "name": n} for p, n in zip(params, names)], lr=0.0, eps=1e-15)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    opt.step()
    return opt, f


@pytest.mark.parametrize("P", (1, 65, 1000))
def test_reset_caps_the_filtered_opacity(P):
    import fused_filter3d as ff
    opt, f = _optimizer(P, seed=30 + P)
    ps = [g["params"][0] for g in opt.param_groups]
    before = [p.detach().cpu().clone() for p in ps]
    moments = [(opt.state[p]["exp_avg"].cpu().clone(), opt.state[p]["exp_avg_sq"].cpu().clone()) for p in ps]
    steps = [opt.state[p]["step"] for p in ps]
    cap = 0.01
    want, changed = ref.reset_logits(before[3], before[4], f, cap)
    sig = torch.sigmoid(before[3].double())
    _, _, coef = ref.activations(before[3], before[4], f)
    below = sig < (cap / coef) * (1 - 1e-6)
    ret = ff.reset_opacity(opt, f.to(DEV), max_opacity=cap)
    assert ret is ps[3]
    got = ps[3].detach().cpu()
    assert torch.equal(got[below].view(torch.int32), before[3][below].view(torch.int32))       # below the cap: the bits stay
    d = ref.ulps(got, want)[~below]
    print(f"P = {P}: {int((~below).sum())} rows at or above the cap, {int((d == 0).sum())} of them 0 ulp, largest {int(d.max()) if d.numel() else 0} ulp")
    assert bool((d <= 1).all())
    if P > 1:
        assert bool(changed.any()) and bool(below.any())
    # the filtered opacity of a changed row is the cap
    o, _, _ = ref.activations(got, before[4], f)
    assert float(o.max()) <= cap * (1 + 1e-5)
    for k, p in enumerate(ps):
        m, v = opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu()
        if k == 3:
            assert bool((m == 0).all()) and bool((v == 0).all()) and not bool(torch.signbit(m).any())
        else:
            assert torch.equal(p.detach().cpu(), before[k]) and torch.equal(m, moments[k][0]) and torch.equal(v, moments[k][1])
        assert opt.state[p]["step"] == steps[k]


@pytest.mark.parametrize("P", (1, 65, 1000))
def test_baked_leaves_are_the_rounded_float64_values(P):
    import fused_filter3d as ff
    opacity, scaling, f, _, _ = _activation_case(P)
    dl, dls, df = (t.to(DEV) for t in (opacity, scaling, f))
    lo, lsc = _padded(P, 1), _padded(P, 3)
    ff._run("gsr_filter3d_bake", P, dl.data_ptr(), dls.data_ptr(), df.data_ptr(), lo.data_ptr(), lsc.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert _intact(lo, P) and _intact(lsc, P)
    want_l, want_s = ref.baked(opacity, scaling, f)
    ul, us = ref.ulps(lo[:P].cpu(), want_l), ref.ulps(lsc[:P].cpu(), want_s)
    print(f"P = {P}: baked logits {int((ul == 0).sum())} of {P} 0 ulp, log-scales {int((us == 0).sum())} of {3 * P} 0 ulp")
    assert bool((ul <= 1).all()) and bool((us <= 1).all())
    a, b = ff.baked_leaves(dl, dls, df)
    assert torch.equal(a, lo[:P]) and torch.equal(b, lsc[:P])
    # a viewer that applies the plain activations to the baked leaves sees the filtered ones
    o, s, _ = ref.activations(opacity, scaling, f)
    assert float(((torch.sigmoid(a.double().cpu()) - o).abs() / o).max()) <= 1e-5 and float(((torch.exp(b.double().cpu()) - s).abs() / s).max()) <= 1e-5


# ---- render(filter_3d=) ----
@pytest.mark.parametrize("antialiasing", (False, True))
@pytest.mark.parametrize("fused", (False, True))
def test_render_applies_the_filtered_activations(fused, antialiasing):
    import fused_filter3d as ff
    import gaussian_renderer
    import gsr_model
    import gsr_scene
    from diff_gaussian_rasterization import GaussianRasterizer
    scene = gsr_scene.make_scene(200, -2.0, sh_degree=3, seed=5)
    cam = gsr_scene.make_camera(32, 32)
    camd = cam._replace(world_view_transform=cam.world_view_transform.to(DEV), full_proj_transform=cam.full_proj_transform.to(DEV),
                        camera_center=cam.camera_center.to(DEV))
    bg = scene.bg.to(DEV)
    pipe = gsr_model.pipeline_params(fused_activations=fused)
    f = (0.01 + 0.05 * torch.rand(200, 1, generator=torch.Generator().manual_seed(6))).to(DEV)
    dpix = torch.randn(3, 32, 32, generator=torch.Generator().manual_seed(7)).to(DEV)

    def model():
        return gsr_model.GaussianParams.from_activated(scene.means3D, scene.shs, scene.scales, scene.rotations, scene.opacities, device=DEV,
                                                       active_sh_degree=3)

    pc = model()
    out = gaussian_renderer.render(camd, pc, pipe, bg, antialiasing=antialiasing, filter_3d=f)
    (out["render"] * dpix).sum().backward()

    # the rasterizer fed the filtered activations, with detached inputs: its own gradients w.r.t. opacities and scales
    pc2 = model()
    o, s = ff.filtered_activations(pc2._opacity, pc2._scaling, f)
    od, sd = o.detach().requires_grad_(True), s.detach().requires_grad_(True)
    settings = gaussian_renderer._settings_for(camd, pc2, pipe, bg, 1.0)
    means2D = torch.zeros_like(pc2.get_xyz, requires_grad=True)
    direct = GaussianRasterizer(raster_settings=settings, antialiasing=antialiasing)(
        means3D=pc2.get_xyz, means2D=means2D, opacities=od, shs=pc2.get_features, colors_precomp=None, scales=sd, rotations=pc2.get_rotation,
        cov3D_precomp=None)
    assert torch.equal(out["render"], direct[0]) and torch.equal(out["radii"], direct[1]) and int((direct[1] > 0).sum()) > 50
    (direct[0] * dpix).sum().backward()
    torch.autograd.backward((o, s), (od.grad, sd.grad))
    assert torch.equal(pc._opacity.grad, pc2._opacity.grad) and torch.equal(pc._scaling.grad, pc2._scaling.grad)
    assert float(pc._opacity.grad.abs().max()) > 0 and float(pc._scaling.grad.abs().max()) > 0
    assert torch.equal(pc._xyz.grad, pc2._xyz.grad) and torch.equal(out["viewspace_points"].grad, means2D.grad)

    # the filter changes the picture, and None is the call without the keyword
    plain = gaussian_renderer.render(camd, model(), pipe, bg, antialiasing=antialiasing)
    none = gaussian_renderer.render(camd, model(), pipe, bg, antialiasing=antialiasing, filter_3d=None)
    assert torch.equal(plain["render"], none["render"]) and torch.equal(plain["radii"], none["radii"])
    assert not torch.equal(plain["render"], out["render"])
