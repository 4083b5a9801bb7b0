"""GPU: fixed-budget (MCMC) training (include/gsr_mcmc.h, fused_mcmc.py) against tests/torch_mcmc.py in float64.

Noise, P in {1, 63, 257, 1000} (a lone lane, a wave that is not full, a workgroup and a lane, several workgroups with a remainder):
the error of the displacement per Gaussian, normalised by ||Sigma||_F ||eps|| gate scaler, is at most 2 e_stock + 2^-22, e_stock the
same figure of the stock fp32 sequence evaluated here on the CPU for the same inputs (the factor 2 for another operation order, the
floor for inputs where the stock sequence happens to be exact).  Over all Gaussians both figures are 1 wherever an fp32 gate
underflows to exactly 0 against a reference of 1e-39, so the same bar is also held over the Gaussians whose reference gate is at
least 1e-30, where it says something.  Below that gate a row keeps its bits.
Relocation: the recomputed logit and log-scales within 1 fp32 ulp of the float64 reference rounded to fp32 (the kernel computes in
double and rounds once; device and host libm may differ in the last bits of the double, which can move the rounding by one unit);
everything else bit for bit.
Regulariser: value within (elements per thread + log2(workgroup size) + 4) 2^-24 relative (a fixed-order sum of positive terms),
every gradient element within 8 * 2^-24 relative."""
import math

import numpy as np
import pytest
import torch

import torch_mcmc as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SCALER = 0.8          # noise_lr 5e5 * lr_xyz 1.6e-6
MIN_OPACITY = 0.005
_cache = {}


def _noise_case(P):
    """-> leaves and noise on the device, the float64 displacement, gate and ||Sigma||_F, the stock fp32 sequence's normalised error
    per Gaussian; computed once and shared, never written to"""
    if P not in _cache:
        xyz, _, _, opacity, scaling, rotation = ref.make_leaves(P, seed=P)
        eps = torch.randn(P, 3, generator=torch.Generator().manual_seed(77 + P))
        d64, g, fro = ref.noise_displacement(opacity, scaling, rotation, eps, SCALER)
        stock = ref.stock_noise_displacement(opacity, scaling, rotation, eps, SCALER)
        e_stock = ref.normalised_noise_error(stock, d64, g, fro, eps, SCALER)
        _cache[P] = tuple(t.to(DEV) for t in (xyz, opacity, scaling, rotation, eps)) + (d64, g, fro, e_stock, eps)
    return _cache[P]


@pytest.mark.parametrize("P", (1, 63, 257, 1000))
def test_noise_matches_the_float64_reference(P):
    import fused_mcmc as fm
    xyz, opacity, scaling, rotation, eps, d64, g, fro, e_stock, eps_cpu = _noise_case(P)
    # run 1: from zero, the result is the displacement itself
    d1 = fm.inject_noise(torch.zeros_like(xyz), opacity, scaling, rotation, SCALER, noise=eps)
    assert bool(torch.isfinite(d1).all())
    err = ref.normalised_noise_error(d1.cpu(), d64, g, fro, eps_cpu, SCALER)
    live = g >= 1e-30
    for name, sel in (("all", torch.ones_like(live)), ("gate >= 1e-30", live)):
        if not bool(sel.any()):
            continue
        achieved, stock = float(err[sel].max()), float(e_stock[sel].max())
        print(f"P = {P}, {name} ({int(sel.sum())} Gaussians): stock fp32 {stock:.2e}, kernel {achieved:.2e}, bar {2 * stock + 2.0 ** -22:.2e}")
        assert achieved <= 2 * stock + 2.0 ** -22, (name, achieved, stock)
    if P >= 257:
        assert bool(live.any()) and bool((~live).any()) and float(g.max()) > 0.5
    # run 2: real positions, the same noise: xyz + displacement formed in fp32, bit for bit
    moved = fm.inject_noise(xyz.clone(), opacity, scaling, rotation, SCALER, noise=eps)
    assert torch.equal(moved, xyz + d1)
    assert float(xyz.abs().min()) >= 1e-3 and torch.equal(moved[~live.to(DEV)], xyz[~live.to(DEV)])   # |d| < 1e-27 there: no bit moves
    assert bool((d1[g.to(DEV) < 1e-40] == 0).all())
    # again: the same bits
    assert torch.equal(fm.inject_noise(xyz.clone(), opacity, scaling, rotation, SCALER, noise=eps), moved)


def test_noise_drawn_by_the_wrapper_follows_the_generator():
    import fused_mcmc as fm
    xyz, opacity, scaling, rotation, *_ = _noise_case(257)
    gen = torch.Generator(device=DEV)
    a = fm.inject_noise(xyz.clone(), opacity, scaling, rotation, SCALER, generator=gen.manual_seed(5))
    eps = torch.randn((257, 3), dtype=torch.float32, device=DEV, generator=gen.manual_seed(5))
    assert torch.equal(a, fm.inject_noise(xyz.clone(), opacity, scaling, rotation, SCALER, noise=eps)) and not torch.equal(a, xyz)
    x = xyz.clone().requires_grad_(True)   # a leaf that requires grad is changed in place all the same, and the return is the argument
    assert fm.inject_noise(x, opacity, scaling, rotation, SCALER, noise=eps) is x and torch.equal(x.detach(), a)


# ---- relocation ----
HI, TOP, LO, MANY, ONCE = 3, 4, 5, 6, 7   # source rows: o = 0.999, a logit of 33 (the upper clamp), o = 0.006, named 60 times, named once


def _relocation_case(rest, D, grow=0):
    """-> (leaves [P + grow rows], dst, src) on the CPU.  Sources lie below row 130, destinations from row 130 on."""
    P = 257
    leaves = ref.make_leaves(P, rest=rest, seed=10 * rest + D, logit_range=6.0)
    leaves[3][HI, 0] = math.log(0.999 / 0.001)
    leaves[3][TOP, 0] = 33.0
    leaves[3][LO, 0] = math.log(0.006 / 0.994)
    g = torch.Generator().manual_seed(D)
    if D == 120:   # MANY 60 times: n clamps at 51; LO 50 times: n = 51 and o' falls below min_opacity
        src = torch.cat([torch.full((60,), MANY), torch.full((50,), LO), torch.tensor([ONCE, HI, HI, HI, TOP]),
                         torch.randint(8, 130, (5,), generator=g)])
    elif D == 5:
        src = torch.tensor([MANY, LO, HI, TOP, MANY])
    else:
        src = torch.tensor([ONCE])
    src = src[torch.randperm(D, generator=g)]
    if grow:
        leaves = [torch.cat([t, torch.zeros((grow,) + tuple(t.shape[1:]))]) for t in leaves]
        dst = torch.arange(P, P + grow)
        assert grow == D
    else:
        dst = 130 + torch.randperm(127, generator=g)[:D]
    return leaves, dst, src


def _moments(leaves, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(t.shape, generator=g), torch.rand(t.shape, generator=g)) for t in leaves]


def _ulps(got, want):
    """|got - want| in units of want's spacing, float32"""
    got, want = got.numpy().astype(np.float32), want.numpy().astype(np.float32)
    return float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64), initial=0.0))


def _assert_relocated(got_params, got_moments, leaves, moments, dst, src, zero):
    want_params, want_moments, exact = ref.relocate(leaves, moments, dst, src, 3, 4, MIN_OPACITY, zero)
    named = torch.cat([dst, src]).unique()
    other = torch.ones(leaves[0].shape[0], dtype=torch.bool)
    other[named] = False
    for k, (got, want) in enumerate(zip(got_params, want_params)):
        got = got.cpu()
        if k in (3, 4):
            worst = _ulps(got[named], want[named])
            print(f"group {k}: recomputed rows within {worst:.2f} ulp of the float64 reference")
            assert worst <= 1.0, (k, worst)
            assert torch.equal(got[other], leaves[k][other]), k
            assert torch.equal(got[dst], got[src]), k          # a copy carries its source's new bits
        else:
            assert torch.equal(got, want), k                   # dst rows the source's bits, every other row its own
    for k, (got, want) in enumerate(zip(got_moments, want_moments)):
        if want is None:
            assert got is None
            continue
        for a, b in zip(got, want):
            a = a.cpu()
            assert torch.equal(a, b), k
            if zero:
                assert bool((a[src] == 0).all()) and not bool(torch.signbit(a[src]).any()), k
    return exact


RELOCATIONS = [(15, 1, "all", True), (15, 5, "all", True), (15, 120, "all", True), (0, 1, "all", False), (0, 5, "none", True),
               (0, 120, "all", True), (15, 120, "none", True), (15, 120, "some", False), (15, 120, "some", True)]


@pytest.mark.parametrize("rest,D,with_moments,zero", RELOCATIONS)
def test_relocation_matches_the_float64_reference(rest, D, with_moments, zero):
    import fused_mcmc as fm
    leaves, dst, src = _relocation_case(rest, D)
    moments = _moments(leaves, D)
    if with_moments == "none":
        moments = [None] * 6
    elif with_moments == "some":   # the features without moments
        moments[1] = moments[2] = None

    def run():
        params = [t.to(DEV) for t in leaves]
        moms = [None if m is None else (m[0].to(DEV), m[1].to(DEV)) for m in moments]
        fm.relocate([(p, None if m is None else m[0], None if m is None else m[1]) for p, m in zip(params, moms)], dst.to(DEV), src.to(DEV),
                    min_opacity=MIN_OPACITY, zero_src_moments=zero)
        return params, moms

    params, moms = run()
    exact = _assert_relocated(params, moms, leaves, moments, dst, src, zero)
    if D == 120:   # the cases the sources were built for
        counts = torch.bincount(src)
        assert int(counts[MANY]) == 60 and int(counts[LO]) == 50 and int(counts[ONCE]) == 1
        assert exact[LO][0] == math.log(MIN_OPACITY / (1 - MIN_OPACITY)) and exact[TOP][0] == math.log(ref.OPACITY_MAX / (1 - ref.OPACITY_MAX))
        lo, top = float(params[3][LO, 0]), float(params[3][TOP, 0])
        assert abs(lo - exact[LO][0]) <= 5e-7 and abs(top - exact[TOP][0]) <= 2e-6 and math.isfinite(top)
    again, moms_again = run()
    for a, b in zip(params, again):
        assert torch.equal(a, b)
    for a, b in zip(moms, moms_again):
        assert a is None or (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))


@pytest.mark.parametrize("rest", (15, 0))
def test_growing_the_set_is_the_same_call(rest):
    import fused_mcmc as fm
    leaves, dst, src = _relocation_case(rest, 5, grow=5)
    moments = [(m * (torch.arange(262) < 257).reshape([-1] + [1] * (m.dim() - 1)), v * (torch.arange(262) < 257).reshape([-1] + [1] * (v.dim() - 1)))
               for m, v in _moments(leaves, 3)]   # zero moments for the new rows
    params = [t.to(DEV) for t in leaves]
    moms = [(m.to(DEV), v.to(DEV)) for m, v in moments]
    fm.relocate([(p, m, v) for p, (m, v) in zip(params, moms)], dst.to(DEV), src.to(DEV), min_opacity=MIN_OPACITY, zero_src_moments=False)
    _assert_relocated(params, moms, leaves, moments, dst, src, False)
    assert all(bool((m[257:] == 0).all()) and bool((v[257:] == 0).all()) for m, v in moms)


def _optimizer(leaves, steps=1):
    from fused_params import FusedAdam
    import fused_mcmc as fm
    params = [torch.nn.Parameter(t.to(DEV)) for t in leaves]
    opt = FusedAdam([{"params": [p], "lr": 1e-3, "name": n} for p, n in zip(params, fm.LEAF_NAMES)], lr=0.0, eps=1e-15)
    g = torch.Generator().manual_seed(11)
    for _ in range(steps):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g).to(DEV)
        opt.step()
    return opt


def _state(opt):
    """-> ([param], [(exp_avg, exp_avg_sq)], [step]) as CPU copies, in group order"""
    ps = [g["params"][0] for g in opt.param_groups]
    return ([p.detach().cpu().clone() for p in ps], [(opt.state[p]["exp_avg"].cpu().clone(), opt.state[p]["exp_avg_sq"].cpu().clone()) for p in ps],
            [opt.state[p]["step"] for p in ps])


def test_relocation_through_the_optimizer_and_its_refusals():
    import fused_mcmc as fm
    leaves, dst, src = _relocation_case(15, 120)
    opt = _optimizer(leaves, steps=2)
    before, moments, steps = _state(opt)
    # no entry: nothing happens
    fm.relocate(opt, dst[:0].to(DEV), src[:0].to(DEV))
    after, moments_after, _ = _state(opt)
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(moments, moments_after))
    # the preconditions, checked on request
    with pytest.raises(RuntimeError, match="twice"):
        fm.relocate(opt, torch.tensor([200, 201, 200], device=DEV), torch.tensor([1, 2, 3], device=DEV))
    with pytest.raises(RuntimeError, match="both in dst and in src"):
        fm.relocate(opt, torch.tensor([200, 201], device=DEV), torch.tensor([1, 200], device=DEV))
    with pytest.raises(RuntimeError, match="outside"):
        fm.relocate(opt, torch.tensor([200, 257], device=DEV), torch.tensor([1, 2], device=DEV))
    with pytest.raises(RuntimeError, match="outside"):
        fm.relocate(opt, torch.tensor([200, 201], device=DEV), torch.tensor([1, -1], device=DEV))
    after, moments_after, _ = _state(opt)
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(moments, moments_after))
    fm.relocate(opt, dst.to(DEV), src.to(DEV), min_opacity=MIN_OPACITY)
    ps = [g["params"][0] for g in opt.param_groups]
    _assert_relocated([p.detach() for p in ps], [(opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in ps], before, moments, dst, src, True)
    assert [opt.state[p]["step"] for p in ps] == steps == [2] * 6


# ---- regulariser ----
@pytest.mark.parametrize("P", (1, 257, 5000))
def test_regulariser_matches_the_float64_reference(P):
    import fused_mcmc as fm
    _, _, _, opacity, scaling, _ = ref.make_leaves(P, seed=P, logit_range=12.0)
    w_o, w_s = 0.01, 0.02
    val64, do64, ds64 = ref.regularizer(opacity, scaling, w_o, w_s)
    l, s = opacity.to(DEV).requires_grad_(True), scaling.to(DEV).requires_grad_(True)
    val, raw = fm.regularizer_and_grads(l.detach(), s.detach(), w_o, w_s)
    rel = abs(float(val[0]) - float(val64)) / float(val64)
    bar = (fm.REG_ELEMS_PER_THREAD + math.log2(fm.REG_THREADS) + 4) * 2.0 ** -24
    e_o = float(((raw["opacity"].double().cpu() - do64).abs() / do64).max())
    e_s = float(((raw["scaling"].double().cpu() - ds64).abs() / ds64).max())
    print(f"P = {P}: value rel {rel:.2e} (bar {bar:.2e}); d/dopacity {e_o / 2.0 ** -24:.2f}, d/dscaling {e_s / 2.0 ** -24:.2f} units of 2^-24 (bar 8)")
    assert rel <= bar
    assert e_o <= 8 * 2.0 ** -24 and e_s <= 8 * 2.0 ** -24
    if P >= 257:
        assert float(opacity.abs().max()) > 9.0   # where y (1 - y) has lost its digits
    # the autograd Function: a scalar, scaled by the upstream gradient, accumulating into .grad
    loss = fm.regularizer(l, s, w_o, w_s)
    assert loss.dim() == 0 and float(loss.detach()) == float(val[0])
    (3.0 * loss).backward()
    assert torch.equal(l.grad, 3.0 * raw["opacity"]) and torch.equal(s.grad, 3.0 * raw["scaling"])
    fm.regularizer(l, s, w_o, w_s).backward()
    assert torch.equal(l.grad, 3.0 * raw["opacity"] + raw["opacity"]) and torch.equal(s.grad, 3.0 * raw["scaling"] + raw["scaling"])
    # only what needs a gradient gets one, and the bits repeat
    only = fm.regularizer(l.detach(), s, w_o, w_s)
    (g_s,) = torch.autograd.grad(only, s)
    assert torch.equal(g_s, raw["scaling"]) and float(only.detach()) == float(val[0])
    assert not fm.regularizer(l.detach(), s.detach()).requires_grad
    val_b, raw_b = fm.regularizer_and_grads(l.detach(), s.detach(), w_o, w_s)
    assert torch.equal(val, val_b) and torch.equal(raw["opacity"], raw_b["opacity"]) and torch.equal(raw["scaling"], raw_b["scaling"])
    val_c, none = fm.regularizer_and_grads(l.detach(), s.detach(), w_o, w_s, want=())
    assert none == {} and torch.equal(val, val_c)


# ---- helpers ----
def _helper_leaves():
    """P = 1000 with 40 dead rows; every live opacity is at least 0.05, so that no new opacity comes near min_opacity"""
    P = 1000
    leaves = ref.make_leaves(P, rest=3, seed=40, logit_range=6.0)
    leaves[3].clamp_(min=math.log(0.05 / 0.95))
    dead = torch.randperm(P, generator=torch.Generator().manual_seed(41))[:40]
    leaves[3][dead] = -7.0
    return leaves, dead


def test_relocate_dead_moves_every_dead_row_onto_a_live_one():
    import fused_mcmc as fm
    leaves, dead = _helper_leaves()
    a, b = _optimizer(leaves), _optimizer(leaves)
    seen = []
    real = fm.relocate

    def spy(groups, dst, src, **kw):
        seen.append((dst.clone(), src.clone(), kw))
        return real(groups, dst, src, **kw)

    fm.relocate = spy
    try:
        moved = fm.relocate_dead(a, min_opacity=MIN_OPACITY, generator=torch.Generator(device=DEV).manual_seed(3))
    finally:
        fm.relocate = real
    assert moved == 40 and len(seen) == 1
    dst, src, kw = seen[0]
    assert kw == dict(min_opacity=MIN_OPACITY, zero_src_moments=True, check=False)
    assert sorted(dst.tolist()) == sorted(dead.tolist()) and not set(src.tolist()) & set(dead.tolist())
    opac = torch.sigmoid(dict((g["name"], g["params"][0]) for g in a.param_groups)["opacity"].detach())
    assert float(opac.min()) > MIN_OPACITY
    fm.relocate(b, dst, src, min_opacity=MIN_OPACITY, zero_src_moments=True, check=True)   # the draw keeps the preconditions
    (pa, ma, sa), (pb, mb, sb) = _state(a), _state(b)
    assert all(torch.equal(x, y) for x, y in zip(pa, pb)) and sa == sb == [1] * 6
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(ma, mb))
    assert fm.relocate_dead(a, min_opacity=MIN_OPACITY) == 0


def test_add_new_grows_the_set_and_the_optimizer_steps_on():
    import fused_mcmc as fm
    leaves, _ = _helper_leaves()
    leaves[3].clamp_(min=math.log(0.05 / 0.95))   # nothing dead here
    opt = _optimizer(leaves)
    before, moments, _ = _state(opt)
    gen = torch.Generator(device=DEV).manual_seed(4)
    assert fm.add_new(opt, cap_max=1030, generator=gen) == min(1030, math.ceil(1.05 * 1000)) - 1000 == 30
    after, moments_after, steps = _state(opt)
    assert steps == [1] * 6
    for k, (old, new) in enumerate(zip(before, after)):
        assert new.shape == (1030,) + tuple(old.shape[1:])
        if k not in (3, 4):
            assert torch.equal(new[:1000], old)
        m, v = moments_after[k]
        assert torch.equal(m[:1000], moments[k][0]) and torch.equal(v[:1000], moments[k][1])      # no moment is zeroed ...
        assert bool((m[1000:] == 0).all()) and bool((v[1000:] == 0).all())                        # ... and the new rows start at zero
    assert bool((after[0][1000:] != 0).any()) and bool((after[3][1000:] != 0).all())
    assert fm.add_new(opt, cap_max=1030, generator=gen) == 0
    params = [g["params"][0] for g in opt.param_groups]
    for p in params:
        assert p.requires_grad and p.shape[0] == 1030
        p.grad = torch.ones_like(p)
    opt.step()
    stepped, _, steps = _state(opt)
    assert steps == [2] * 6 and all(bool(torch.isfinite(s).all()) and not torch.equal(s, a) for s, a in zip(stepped, after))
    assert fm.add_new(opt, cap_max=10 ** 6, generator=gen) == math.ceil(1.05 * 1030) - 1030
