"""GPU: the one-launch Adam (csrc/optimizer.hip, fused_params.FusedAdam) against tests/torch_adam.py in float64.

Bar, per tensor (param, exp_avg, exp_avg_sq) and per group: max|got - ref64| <= max(2^-23, 3 n32) max|ref64|, n32 the same normalised
distance of the float32 run of the reference from its float64 run (the rule of test_loss.py and test_loss_ext_gpu.py; 2^-23 is one
fp32 ulp of the largest element).  n32 and the achieved value are printed for every tensor.

Conditions, asserted on the CPU before anything is compared: (a) every non-zero gradient has |g| >= 1e-13, so that (1 - b2) g^2 stays a
normal fp32 number; (b) for every group the median |p_T - p_0| of the float64 reference (over the rows that are updated) is at least
50 bars, so that a wrong lr or a wrong bias correction cannot hide inside the bar.

Inputs: the recipe of test_fused_params_gpu._adam_problem -- randn parameters, randn 10^k gradients with k in [-6, 0] drawn per group
and step, the reference's six learning rates, eps 1e-15, six steps; a state that has lived has exp_avg = 1e-3 randn, exp_avg_sq =
1e-5 rand.  Every tensor the kernel sees lies inside a larger buffer filled with NaN: 4 floats in (16-byte aligned, the float4 path)
or 1 float in (data_ptr() % 16 == 4, the scalar path), and the guard elements on both sides must still be NaN afterwards.

In a group of one to five elements n32 is a sample of a handful of roundings and can come out near 0 while another, equally good
fp32 evaluation lands a full ulp away after six steps.  The seeds of those groups (_edge_groups, _many_groups) were therefore
picked on the CPU alone, before any GPU run: an fp32 evaluation in the kernel's operation order, once with and once without fused
multiply-adds, stays below 0.4 of the bar for them (it exceeds the bar for about one seed in five)."""
import pytest
import torch

import torch_adam as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 1e-15
STEPS = 6
NAMES = ("param", "exp_avg", "exp_avg_sq")
SLOTS = ("param", "grad", "exp_avg", "exp_avg_sq")
LRS = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=2.5e-3 / 20, opacity=0.05, scaling=5e-3, rotation=1e-3)   # arguments/__init__.py:71-81
ZERO_ROWS = (2, 5, -3)     # of "scaling": zero gradient in every step and zero moments
ALIGNED = dict.fromkeys(SLOTS, 4)
_cache = {}


def _shapes(P):
    return dict(xyz=(P, 3), f_dc=(P, 1, 3), f_rest=(P, 15, 3), opacity=(P, 1), scaling=(P, 3), rotation=(P, 4))


def _group(name, shape, lr, g, step0=0, betas=(0.9, 0.999), eps=EPS, has_grad=True):
    """One single-tensor group as CPU fp32 tensors: parameter, one gradient per step, the moments of a state that has lived"""
    p0 = torch.randn(shape, generator=g)
    grads = [torch.randn(shape, generator=g) * 10 ** float(torch.randint(-6, 1, (1,), generator=g)) for _ in range(STEPS)]
    m0 = 1e-3 * torch.randn(shape, generator=g) if step0 else None
    v0 = 1e-5 * torch.rand(shape, generator=g) if step0 else None
    return dict(name=name, p0=p0, grads=grads if has_grad else None, m0=m0, v0=v0, step0=step0, lrs=[lr] * STEPS, betas=betas, eps=eps)


def _product_groups(P, seed, step0):
    """The six product groups; the xyz lr changes before the fourth step (update_learning_rate()), the fifth opacity gradient is all
    zero (the momentum still moves the parameter) and ZERO_ROWS of scaling never see a gradient and have no moments."""
    g = torch.Generator().manual_seed(seed)
    groups = [_group(k, s, LRS[k], g, step0) for k, s in _shapes(P).items()]
    by = {q["name"]: q for q in groups}
    by["xyz"]["lrs"] = [1.6e-4] * 3 + [0.9e-4] * 3
    by["opacity"]["grads"][4] = torch.zeros_like(by["opacity"]["p0"])
    rows = list(ZERO_ROWS)
    for t in by["scaling"]["grads"] + ([by["scaling"]["m0"], by["scaling"]["v0"]] if step0 else []):
        t[rows] = 0.0
    return groups


def _nerr(a, b):
    return float((a.double().cpu() - b.double()).abs().max() / max(float(b.abs().max()), 1e-30))


def _reference(key, groups, visible=None):
    """-> per group (r64, r32, n32) with r = (param, exp_avg, exp_avg_sq); computed once per key, shared, never written to.  The two
    conditions of the module docstring are asserted here."""
    if key in _cache:
        return _cache[key]
    out = []
    rows = None if visible is None else visible.cpu().bool()
    for q in groups:
        if q["grads"] is None or q["p0"].numel() == 0:
            out.append(None)
            continue
        for gr in q["grads"]:      # (a)
            assert bool((gr[gr != 0].abs() >= 1e-13).all()), (key, q["name"])
        kw = dict(betas=q["betas"], eps=q["eps"], exp_avg=q["m0"], exp_avg_sq=q["v0"], step0=q["step0"], visible=rows)
        r64 = ref.adam_steps(q["p0"], q["grads"], q["lrs"], dtype=torch.float64, **kw)
        r32 = ref.adam_steps(q["p0"], q["grads"], q["lrs"], dtype=torch.float32, **kw)
        n32 = tuple(_nerr(b, a) for a, b in zip(r64, r32))
        if rows is None or bool(rows.any()):      # (b)
            bar = max(2.0 ** -23, 3.0 * n32[0]) * float(r64[0].abs().max())
            moved = (r64[0] - q["p0"].double()).abs()
            moved = moved if rows is None else moved[rows]
            ratio = float(moved.flatten().median()) / bar
            print(f"{key} {q['name']}: median |p_T - p_0| = {ratio:.0f} bars")
            assert ratio >= 50.0, (key, q["name"], ratio)
        out.append((r64, r32, n32))
    _cache[key] = out
    return out


def _guarded(t, off):
    """`t` on the device, `off` floats into a NaN-filled buffer with at least 4 floats of guard behind it -> (buffer, view)"""
    n = t.numel()
    buf = torch.full((off + n + 4 + (-(off + n)) % 4,), float("nan"), device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + n].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and (n == 0 or view.data_ptr() == buf.data_ptr() + 4 * off)
    return buf, view


def _run(groups, offs=ALIGNED, radii=None, step_as="tensor", stream=None, steps=STEPS):
    """The steps through FusedAdam, every tensor guarded as `offs` says (floats into its buffer, per slot) -> (optimizer, parameters,
    per group None or {param, exp_avg, exp_avg_sq on the CPU, step, guards: all still NaN, ptrs})"""
    from fused_params import FusedAdam
    bufs, params, spec = [], [], []
    for q in groups:
        zeros = torch.zeros_like(q["p0"])
        b = {"param": _guarded(q["p0"], offs["param"]), "grad": _guarded(zeros, offs["grad"]),
             "exp_avg": _guarded(zeros if q["m0"] is None else q["m0"], offs["exp_avg"]),
             "exp_avg_sq": _guarded(zeros if q["v0"] is None else q["v0"], offs["exp_avg_sq"])}
        p = torch.nn.Parameter(b["param"][1])
        assert p.data_ptr() == b["param"][1].data_ptr() and p.is_contiguous()
        bufs.append(b)
        params.append(p)
        spec.append({"params": [p], "lr": q["lrs"][0], "name": q["name"], "betas": q["betas"], "eps": q["eps"]})
    opt = FusedAdam(spec, lr=0.0, eps=EPS)
    for q, b, p in zip(groups, bufs, params):
        step0 = torch.tensor(float(q["step0"])) if step_as == "tensor" else int(q["step0"])
        opt.state[p] = {"step": step0, "exp_avg": b["exp_avg"][1], "exp_avg_sq": b["exp_avg_sq"][1]}
    torch.cuda.synchronize()
    for it in range(steps):
        for q, b, p, grp in zip(groups, bufs, params, opt.param_groups):
            grp["lr"] = q["lrs"][it]
            if q["grads"] is not None:
                b["grad"][1].copy_(q["grads"][it])
                p.grad = b["grad"][1]
        torch.cuda.synchronize()
        if stream is None:
            opt.step(visible_radii=radii)
        else:
            with torch.cuda.stream(stream):
                opt.step(visible_radii=radii)
        torch.cuda.synchronize()
    out = []
    for q, b, p in zip(groups, bufs, params):
        n = q["p0"].numel()
        guards = all(bool(torch.isnan(buf[:offs[s]]).all()) and bool(torch.isnan(buf[offs[s] + n:]).all()) and buf.numel() > offs[s] + n
                     for s, (buf, _) in b.items())
        st = opt.state[p]
        out.append(dict(param=p.data.cpu().clone(), exp_avg=st["exp_avg"].cpu().clone(), exp_avg_sq=st["exp_avg_sq"].cpu().clone(),
                        step=st["step"], guards=guards, ptrs={s: view.data_ptr() for s, (_, view) in b.items()}))
    return opt, params, out


def _check(tag, groups, got, want, rows=None):
    """Every figure is printed, then every tensor of every group is held to the bar; rows outside `rows` must have kept their bits."""
    fails = []
    for q, o, w in zip(groups, got, want):
        assert o["guards"], (tag, q["name"], "a guard element was written")
        if w is None:
            continue
        r64, _, n32 = w
        for name, a, n in zip(NAMES, r64, n32):
            ach, bar = _nerr(o[name], a), max(2.0 ** -23, 3.0 * n)
            print(f"{tag} {q['name']} {name}: n32 = {n:.2e} achieved = {ach:.2e} bar = {bar:.2e}")
            if not (o[name].shape == a.shape and bool(torch.isfinite(o[name]).all()) and ach <= bar):
                fails.append((q["name"], name, ach, bar))
        if rows is not None:
            before = dict(param=q["p0"], exp_avg=q["m0"], exp_avg_sq=q["v0"])
            for name in NAMES:
                assert torch.equal(o[name][~rows], before[name][~rows]), (tag, q["name"], name, "an invisible row changed")
    assert not fails, (tag, fails)


# ---- 1. dense, against float64 ----

@pytest.mark.parametrize("step0,step_as", [(0, "int"), (999, "tensor"), (29999, "int")])
def test_dense_steps_match_the_float64_reference(step0, step_as):
    """P = 1366: xyz has 4098 elements (five blocks of 1024, a scalar tail of 2); f_rest is (P, 15, 3)"""
    P = 1366
    groups = _product_groups(P, 21 + step0, step0)
    assert _shapes(P)["xyz"] == (P, 3) and P * 3 == 4 * 1024 + 2
    want = _reference(("dense", step0), groups)
    _, _, got = _run(groups, step_as=step_as)
    _check(f"dense step0={step0}", groups, got, want)
    for o in got:
        assert int(o["step"]) == step0 + STEPS
    # a row without moments and without a gradient keeps its bits
    sc = next(i for i, q in enumerate(groups) if q["name"] == "scaling")
    rows = list(ZERO_ROWS)
    assert torch.equal(got[sc]["param"][rows], groups[sc]["p0"][rows])
    assert bool((got[sc]["exp_avg"][rows] == 0).all()) and bool((got[sc]["exp_avg_sq"][rows] == 0).all())
    assert not torch.equal(got[sc]["param"][1], groups[sc]["p0"][1])


# ---- 2. block and vector edges ----

EDGE_NUMEL = (1, 2, 3, 4, 5, 1023, 1024, 1025)
EDGE_LRS = (2e-3, 0.05, 5e-3, 1e-3, 2.5e-3, 1.6e-4, 1.25e-4, 1e-2)


def _edge_groups(seed=306):
    g = torch.Generator().manual_seed(seed)
    return [_group(f"n{n}", (n,), lr, g, step0=999) for n, lr in zip(EDGE_NUMEL, EDGE_LRS)]


def test_one_launch_of_eight_groups_at_the_block_and_vector_edges():
    """numel 1..5 around the float4, 1023..1025 around the 1024-element block, every group with its own lr: an element of a
    neighbouring group, or a guard, that is touched shows"""
    groups = _edge_groups()
    want = _reference("edges", groups)
    _, _, got = _run(groups)
    _check("edges", groups, got, want)
    for o in got:
        assert int(o["step"]) == 999 + STEPS and all(ptr % 16 == 0 for ptr in o["ptrs"].values())


# ---- 3. the unaligned (scalar) path ----

def _unaligned_case():
    groups = _product_groups(1366, 21 + 999, 999)
    return groups, _reference(("dense", 999), groups)


@pytest.mark.parametrize("which", SLOTS + ("all",))
def test_a_pointer_one_float_off_takes_the_scalar_path(which):
    groups, want = _unaligned_case()
    offs = {s: (1 if which in (s, "all") else 4) for s in SLOTS}
    _, _, got = _run(groups, offs=offs)
    for o in got:
        for s in SLOTS:
            assert o["ptrs"][s] % 16 == (4 if offs[s] == 1 else 0), (s, o["ptrs"][s])       # vec_ok == 0
    _check(f"unaligned {which}", groups, got, want)
    if "aligned" not in _cache:
        _cache["aligned"] = _run(groups)[2]
    same = all(torch.equal(a[n], b[n]) for a, b in zip(got, _cache["aligned"]) for n in NAMES)
    print(f"unaligned {which}: bit-identical to the aligned run: {same}")     # not asserted: the two paths may contract differently


# ---- 4. more than 8 groups ----

MANY_SHAPES = ((7, 3), (1,), (1025,), (33, 4), (5, 1, 3), (37, 0, 3), (300, 15, 3), (2,), (1024,), (3,), (129, 3), (64, 4), (1023,),
               (4,), (77, 1), (6, 45), (2049,))
MANY_LRS = (1.6e-4, 0.05, 2.5e-3, 1e-3, 5e-3, 1e-3, 1.25e-4, 0.05, 1e-3, 5e-3, 1.6e-4, 1e-3, 2.5e-3, 0.05, 5e-3, 1.25e-4, 1e-3)


def _many_groups(seed=314):
    g = torch.Generator().manual_seed(seed)
    groups = []
    for i, (shape, lr) in enumerate(zip(MANY_SHAPES, MANY_LRS)):
        betas, eps = ((0.8, 0.99), 1e-8) if i == 3 else (((0.9, 0.999), 1e-8) if i == 13 else ((0.9, 0.999), EPS))
        groups.append(_group(f"g{i}", shape, lr, g, step0=(0, 999, 29999)[i % 3], betas=betas, eps=eps, has_grad=i != 11))
    for q in groups:
        if q["m0"] is None and q["name"] == "g11":
            q["m0"], q["v0"] = torch.zeros_like(q["p0"]), torch.zeros_like(q["p0"])
    return groups


def test_seventeen_groups_an_empty_one_one_without_gradient_and_other_betas():
    """17 single-tensor groups.  Group 5 is (P, 0, 3), group 11 has no gradient (absent from every launch: state and step untouched),
    groups 3 and 13 have other betas / eps and so make batches of their own with the reference taking each group's values: the 14
    others go in launches of 8 and 6, and 3 and 13 in a launch of one group each."""
    from diff_gaussian_rasterization import _C
    groups = _many_groups()
    assert len(groups) == 17 and groups[5]["p0"].numel() == 0 and groups[11]["grads"] is None and groups[11]["step0"] == 29999
    want = _reference("many", groups)
    L = _C.lib()
    real, launches = L.gsr_adam_step, []
    L.gsr_adam_step = lambda n, *a: launches.append(n) or real(n, *a)
    try:
        _, params, got = _run(groups)
    finally:
        L.gsr_adam_step = real
    assert launches == [8, 6, 1, 1] * STEPS, launches
    _check("many", groups, got, want)
    for i, (q, o) in enumerate(zip(groups, got)):
        if i == 11:
            assert torch.is_tensor(o["step"]) and float(o["step"]) == 29999.0 and params[i].grad is None
            assert torch.equal(o["param"], q["p0"]) and torch.equal(o["exp_avg"], q["m0"]) and torch.equal(o["exp_avg_sq"], q["v0"])
        else:
            assert int(o["step"]) == q["step0"] + STEPS, (i, o["step"])
    assert got[5]["param"].shape == (37, 0, 3)


# ---- 5. visible-only, against the masked float64 reference ----

def _radii(P, pattern):
    r = torch.zeros(P, dtype=torch.int32)
    if pattern == "alternating":
        r[::2] = 5
    elif pattern == "last":
        r[-1] = 1
    elif pattern == "first_invisible":
        r[1:] = 9
    elif pattern == "all":
        r[:] = 3
    elif pattern == "negative":       # a negative radius is invisible, like 0
        r[0::3], r[1::3] = 7, -7
    else:
        assert pattern == "none"
    return r


@pytest.mark.parametrize("pattern", ("alternating", "last", "first_invisible", "none", "all", "negative"))
def test_visible_only_against_the_masked_reference(pattern):
    """P = 37 is no multiple of 4, so float4 groups straddle rows of different visibility at every row size (1, 3, 4, 45)"""
    P = 37
    groups = _product_groups(P, 50, 999)
    assert sorted({q["p0"].numel() // P for q in groups}) == [1, 3, 4, 45]
    radii = _radii(P, pattern)
    rows = radii > 0
    assert bool((radii < 0).any()) == (pattern == "negative")
    want = _reference(("visible", pattern), groups, visible=rows)
    _, _, got = _run(groups, radii=radii.to(DEV))
    _check(f"visible {pattern}", groups, got, want, rows=rows)
    for q, o in zip(groups, got):
        assert int(o["step"]) == 999 + STEPS
        if pattern == "none":
            assert torch.equal(o["param"], q["p0"]) and torch.equal(o["exp_avg"], q["m0"]) and torch.equal(o["exp_avg_sq"], q["v0"])
    if pattern == "all":
        _, _, dense = _run(groups)
        for q, o, d in zip(groups, got, dense):
            for name in NAMES:
                assert torch.equal(o[name], d[name]), (q["name"], name)


def test_visible_only_on_the_scalar_path_and_with_an_empty_group():
    """P = 1366 with every pointer one float off: the scalar loop's radii branch.  Then a (P, 0, 3) group (a degree-0 model's
    f_rest) next to xyz: it has no element, and the step is taken."""
    P = 1366
    groups = _product_groups(P, 21 + 999, 999)
    radii = _radii(P, "alternating")
    rows = radii > 0
    want = _reference(("visible", "unaligned"), groups, visible=rows)
    _, _, got = _run(groups, offs=dict.fromkeys(SLOTS, 1), radii=radii.to(DEV))
    assert all(ptr % 16 == 4 for o in got for ptr in o["ptrs"].values())
    _check("visible unaligned", groups, got, want, rows=rows)

    g = torch.Generator().manual_seed(8)
    pair = [_group("xyz", (37, 3), 1.6e-4, g, 999), _group("f_rest", (37, 0, 3), 1.25e-4, g, 999)]
    r37 = _radii(37, "alternating")
    want = _reference(("visible", "empty"), pair, visible=r37 > 0)
    _, _, got = _run(pair, radii=r37.to(DEV))
    _check("visible empty", pair, got, want, rows=r37 > 0)
    assert [int(o["step"]) for o in got] == [999 + STEPS] * 2


# ---- 6. validation: a refused step leaves the optimizer as it was ----

def _snapshot(opt):
    snap = []
    for grp in opt.param_groups:
        for p in grp["params"]:
            st = opt.state.get(p, {})
            snap.append((p.data.clone(), {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}))
    return snap


def _unchanged(opt, snap):
    i = 0
    for grp in opt.param_groups:
        for p in grp["params"]:
            data, st = snap[i]
            now = opt.state.get(p, {})
            if not torch.equal(p.data, data) or sorted(now) != sorted(st):
                return False
            for k, v in st.items():
                if torch.is_tensor(v):
                    if not (torch.is_tensor(now[k]) and now[k].dtype == v.dtype and torch.equal(now[k], v)):
                        return False
                elif type(now[k]) is not type(v) or now[k] != v:
                    return False
            i += 1
    return True


def test_a_refused_step_touches_no_step_count_parameter_or_moment():
    from diff_gaussian_rasterization import _C
    from fused_params import FusedAdam
    P = 37
    g = torch.Generator().manual_seed(4)
    mk = lambda *s, dev=DEV: torch.nn.Parameter(torch.randn(s, generator=g).to(dev))

    def optimizer(extra):
        """xyz (lived, step a tensor), opacity (lived, step an int), rotation (never stepped), then the group under test"""
        ps = dict(xyz=mk(P, 3), opacity=mk(P, 1), rotation=mk(P, 4), **extra)
        opt = FusedAdam([{"params": [p], "lr": 1e-3, "name": k} for k, p in ps.items()], lr=0.0, eps=EPS)
        for k, p in ps.items():
            p.grad = torch.randn(p.shape, generator=g).to(p.device)
        for k, step in (("xyz", torch.tensor(999.0)), ("opacity", 999)):
            opt.state[ps[k]] = {"step": step, "exp_avg": 1e-3 * torch.randn(ps[k].shape, generator=g).to(DEV),
                                "exp_avg_sq": 1e-5 * torch.rand(ps[k].shape, generator=g).to(DEV)}
        return opt, ps

    radii = torch.ones(P, dtype=torch.int32, device=DEV)
    L = _C.lib()
    real, launches = L.gsr_adam_step, []
    L.gsr_adam_step = lambda n, *a: launches.append(n) or real(n, *a)
    try:
        cases = [
            # the known defect: a tensor with more rows than visible_radii (read past its end), one with fewer, one without rows
            ("more rows", dict(bilagrid=mk(P + 5, 12)), dict(visible_radii=radii), "bilagrid"),
            ("fewer rows", dict(exposure=mk(3, 4)), dict(visible_radii=radii), "exposure"),
            ("no rows", dict(scale=mk()), dict(visible_radii=radii), "scale"),
            ("2-D radii", {}, dict(visible_radii=radii.reshape(P, 1)), "1-D"),
            # the refusals that existed, which used to come after the step counts had been incremented
            ("int64 radii", {}, dict(visible_radii=radii.long()), "int32"),
            ("strided radii", {}, dict(visible_radii=torch.ones(2 * P, dtype=torch.int32, device=DEV)[::2]), "contiguous"),
            ("CPU radii", {}, dict(visible_radii=radii.cpu()), "device"),
            ("non-contiguous parameter", dict(scaling=torch.nn.Parameter(torch.randn(3, P, generator=g).to(DEV).t())), {}, "scaling"),
            ("CPU parameter", dict(scaling=mk(P, 3, dev="cpu")), {}, "no CPU path"),
        ]
        for tag, extra, kw, match in cases:
            opt, ps = optimizer(extra)
            snap = _snapshot(opt)
            with pytest.raises(RuntimeError, match=match):
                opt.step(**kw)
            assert _unchanged(opt, snap), tag
            assert not opt.state.get(ps["rotation"]), tag      # no state was created either
        # moments that a half-done densification edit left at another length
        opt, ps = optimizer({})
        opt.state[ps["opacity"]]["exp_avg_sq"] = opt.state[ps["opacity"]]["exp_avg_sq"][:-1].clone()
        snap = _snapshot(opt)
        with pytest.raises(RuntimeError, match="opacity"):
            opt.step()
        assert _unchanged(opt, snap)
        assert launches == []          # nothing above reached the kernel library
        # and the optimizer that refused is still usable: with a radii of the right length the same call goes through
        opt, ps = optimizer({})
        snap = _snapshot(opt)
        opt.step(visible_radii=radii)
        torch.cuda.synchronize()
        assert launches == [3] and not _unchanged(opt, snap)
        assert [int(opt.state[p]["step"]) for p in ps.values()] == [1000, 1000, 1]
    finally:
        L.gsr_adam_step = real


# ---- 7. repeats and streams ----

def test_two_runs_and_a_side_stream_give_the_same_bits():
    groups = _product_groups(1366, 21, 0)
    _, _, a = _run(groups)
    _, _, b = _run(groups)
    side = torch.cuda.Stream(device=DEV)
    _, _, c = _run(groups, stream=side)
    for q, x, y, z in zip(groups, a, b, c):
        for name in NAMES:
            assert torch.equal(x[name], y[name]), (q["name"], name, "second run")
            assert torch.equal(x[name], z[name]), (q["name"], name, "side stream")
        assert not torch.equal(x["param"], q["p0"]) and z["guards"]
