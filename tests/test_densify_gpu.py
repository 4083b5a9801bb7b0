"""GPU: densification (include/gsr_densify.h, fused_densify.py) against expand() of tests/torch_densify.py.

Every copied word, every moment and every extra: bit for bit; `step` untouched.  The children's log-scales: 0 ulp from
fp32(float64(ls) - log 1.6) -- one exactly rounded double subtraction and one rounding, the same on the host and on the device.  The
children's positions as the noise of test_mcmc_gpu: run from xyz = 0 the result is the displacement, whose error per child, normalised
by ||exp(ls) * n||, is at most 2 e_stock + 2^-22 with e_stock the same figure of the stock fp32 sequence (exp, build_rotation, bmm)
evaluated here on the CPU for the same inputs; run from real positions the result is xyz + that displacement in fp32, bit for bit.
Quaternion norms lie in [0.1, 10], log-scales in [-6, 2] (torch_mcmc.make_leaves).
Sizes: 1, 63, 64, 65 (a lane, a wave and its neighbours), R - 1, R, R + 1 and 4 R + 17 with R = GSR_DENSIFY_PLAN_ROWS (one workgroup
of the plan and its neighbours, several with a remainder), and 256 R + 1 at SH degree 0: one workgroup total more than the scan takes
per loop iteration."""
import math

import pytest
import torch

import torch_densify as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
R = 1024              # GSR_DENSIFY_PLAN_ROWS
SCAN = 256            # GSR_DENSIFY_SCAN_THREADS
_cache = {}


def _case(P, rest, mix=(0.5, 0.15, 0.15, 0.2)):
    """-> (leaves, moments, action, noise) on the CPU, computed once and shared, never written to.  mix: the shares of KEEP, PRUNE,
    CLONE, SPLIT"""
    key = (P, rest, mix)
    if key not in _cache:
        leaves, moments, _ = ref.make_case(P, rest=rest, seed=P % 1000 + rest)
        g = torch.Generator().manual_seed(P + 7)
        action = torch.multinomial(torch.tensor(mix), P, replacement=True, generator=g).to(torch.uint8)
        S = int((action == ref.SPLIT).sum())
        noise = torch.randn(2 * S, 3, generator=g)
        _cache[key] = (leaves, moments, action, noise)
    return _cache[key]


def _densify(leaves, moments, action, noise, extras=(), **kw):
    import fused_densify as fd
    rows = [(p.to(DEV), None if m is None else m[0].to(DEV), None if m is None else m[1].to(DEV)) for p, m in zip(leaves, moments)]
    return fd.densify(rows, action.to(DEV), noise=None if noise is None else noise.to(DEV), extras=[(t.to(DEV), z) for t, z in extras], **kw)


def _assert_contract(got, leaves, moments, action, noise, extras=()):
    """everything but the children's positions bit for bit against expand(); -> (expand's result, the children's positions)"""
    outs, extra_outs, counts = got
    want = ref.expand(leaves, moments, action, noise, extras)
    K, C, S = want["counts"]
    assert counts == (K, C, S)
    first = K + C
    for k, ((p, m, v), w, wm) in enumerate(zip(outs, want["leaves"], want["moments"])):
        p = p.cpu()
        assert p.shape == w.shape and p.dtype == w.dtype, k
        if k == ref.XYZ:
            assert torch.equal(p[:first], w[:first])
        else:
            assert torch.equal(p.view(torch.int32), w.view(torch.int32)), k   # the log-scales of the children among them: 0 ulp
        if wm is None:
            assert m is None and v is None, k
        else:
            assert torch.equal(m.cpu().view(torch.int32), wm[0].view(torch.int32)) and torch.equal(v.cpu().view(torch.int32), wm[1].view(torch.int32)), k
    for k, (t, w) in enumerate(zip(extra_outs, want["extras"])):
        assert t.dtype == w.dtype and torch.equal(t.cpu(), w), k
    return want, outs[ref.XYZ][0].cpu()[first:]


def _assert_children(leaves, action, noise, want, children):
    """the two runs of the docstring"""
    K, C, S = want["counts"]
    if S == 0:
        return
    split = want["src"][K + C:K + C + S]
    zero = [(torch.zeros_like(leaves[ref.XYZ]), None), (leaves[ref.SCALING], None), (leaves[ref.ROTATION], None)]
    outs, _, _ = _densify([t for t, _ in zero], [None] * 3, action, noise, xyz_index=0, scaling_index=1, rotation_index=2)
    d1 = outs[0][0].cpu()[K + C:]
    assert bool(torch.isfinite(d1).all())
    stock = ref.stock_child_displacement(leaves[ref.SCALING][split], leaves[ref.ROTATION][split], noise)
    e_stock = float(((stock.double() - want["d64"]).norm(dim=1) / want["scale"]).max())
    err = float(((d1.double() - want["d64"]).norm(dim=1) / want["scale"]).max())
    print(f"P = {action.numel()}, S = {S}: stock fp32 {e_stock:.2e}, kernel {err:.2e}, bar {2 * e_stock + 2.0 ** -22:.2e}")
    assert err <= 2 * e_stock + 2.0 ** -22, (err, e_stock)
    assert torch.equal(children, leaves[ref.XYZ][split].repeat(2, 1) + d1)


@pytest.mark.parametrize("P", (1, 63, 64, 65, R - 1, R, R + 1, 4 * R + 17))
def test_random_code_mix_matches_the_reference(P):
    leaves, moments, action, noise = _case(P, 15)
    got = _densify(leaves, moments, action, noise)
    want, children = _assert_contract(got, leaves, moments, action, noise)
    _assert_children(leaves, action, noise, want, children)
    again = _densify(leaves, moments, action, noise)
    for a, b in zip(got[0], again[0]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_one_workgroup_total_more_than_the_scan_takes_at_once():
    P = SCAN * R + 1
    leaves, moments, action, noise = _case(P, 0)
    moments = [moments[0], None, None, moments[3], None, None]   # moments on some groups only; features_rest has a row of 0 words
    action = action.clone()
    action[-1] = ref.SPLIT   # the lone row of the last workgroup takes part in every class's tail
    noise = torch.randn(2 * int((action == ref.SPLIT).sum()), 3, generator=torch.Generator().manual_seed(1))
    got = _densify(leaves, moments, action, noise)
    want, children = _assert_contract(got, leaves, moments, action, noise)
    assert math.ceil(P / R) == SCAN + 1 and int(want["src"][-1]) == P - 1
    _assert_children(leaves, action, noise, want, children)


@pytest.mark.parametrize("code", (ref.KEEP, ref.PRUNE, ref.CLONE, ref.SPLIT))
def test_one_code_for_every_row(code):
    P = R + 1
    leaves, moments, _, _ = _case(P, 15)
    action = torch.full((P,), code, dtype=torch.uint8)
    noise = torch.randn(2 * P, 3, generator=torch.Generator().manual_seed(code)) if code == ref.SPLIT else None
    got = _densify(leaves, moments, action, noise)
    want, children = _assert_contract(got, leaves, moments, action, noise)
    assert got[2] == {ref.KEEP: (P, 0, 0), ref.PRUNE: (0, 0, 0), ref.CLONE: (P, P, 0), ref.SPLIT: (0, 0, P)}[code]
    if code == ref.KEEP:
        for (p, m, v), t, (wm, wv) in zip(got[0], leaves, moments):
            assert torch.equal(p.cpu(), t) and torch.equal(m.cpu(), wm) and torch.equal(v.cpu(), wv)
    if code == ref.PRUNE:
        assert all(p.shape == (0,) + tuple(t.shape[1:]) and m.shape == p.shape for (p, m, v), t in zip(got[0], leaves))
    if code == ref.SPLIT:
        _assert_children(leaves, action, noise, want, children)


def test_no_split_needs_no_noise_and_no_named_groups():
    P = R + 1
    leaves, moments, action, _ = _case(P, 15, mix=(0.5, 0.2, 0.3, 0.0))
    got = _densify(leaves, moments, action, None)
    _assert_contract(got, leaves, moments, action, None)
    assert got[2][2] == 0
    # a list that holds no xyz, scaling or rotation entry at all
    got = _densify(leaves[1:3], moments[1:3], action, None, xyz_index=None, scaling_index=None, rotation_index=None)
    src = ref.source_rows(action)[0]
    assert torch.equal(got[0][0][0].cpu(), leaves[1][src]) and torch.equal(got[0][1][0].cpu(), leaves[2][src])
    with pytest.raises(RuntimeError, match="a split needs"):
        _densify(leaves[1:3], moments[1:3], torch.full((P,), ref.SPLIT, dtype=torch.uint8), None, xyz_index=None, scaling_index=None, rotation_index=None)


@pytest.mark.parametrize("rest,with_moments", [(0, "all"), (15, "none"), (15, "some"), (0, "some")])
def test_groups_moments_and_extras(rest, with_moments):
    P = R + 1
    leaves, moments, action, noise = _case(P, rest)
    if with_moments == "none":
        moments = [None] * 6
    elif with_moments == "some":   # the features without moments
        moments = [moments[0], None, None] + moments[3:]
    g = torch.Generator().manual_seed(rest)
    extras = [(torch.rand(P, 1, generator=g), True), (torch.rand(P, generator=g), False),                      # denom zeroed, max_radii2D copied
              (torch.randint(-2 ** 31, 2 ** 31 - 1, (P, 2), generator=g, dtype=torch.int64).to(torch.int32), False),   # an index table
              (torch.randint(1, 100, (P,), generator=g, dtype=torch.int64).to(torch.int32), True)]
    got = _densify(leaves, moments, action, noise, extras)
    want, _ = _assert_contract(got, leaves, moments, action, noise, extras)
    K = want["counts"][0]
    assert not bool(got[1][0][K:].any()) and not bool(torch.signbit(got[1][0][K:]).any()) and not bool(got[1][3][K:].any())
    assert bool(got[1][1][K:].any()) and got[1][2].dtype == torch.int32
    if rest == 0:
        assert got[0][2][0].shape == (sum(want["counts"]) + want["counts"][2], 0, 3)


def _optimizer(leaves, moments, step=2):
    from fused_params import FusedAdam
    import fused_densify as fd
    params = [torch.nn.Parameter(t.to(DEV)) for t in leaves]
    opt = FusedAdam([{"params": [p], "lr": 1e-3, "name": n} for p, n in zip(params, fd.LEAF_NAMES)], lr=0.0, eps=1e-15)
    for p, (m, v) in zip(params, moments):
        opt.state[p] = {"step": step, "exp_avg": m.to(DEV), "exp_avg_sq": v.to(DEV)}
    return opt


def _state(opt):
    ps = [g["params"][0] for g in opt.param_groups]
    return ([p.detach().cpu().clone() for p in ps], [(opt.state[p]["exp_avg"].cpu().clone(), opt.state[p]["exp_avg_sq"].cpu().clone()) for p in ps],
            [opt.state[p]["step"] for p in ps])


def test_a_code_above_three_raises_and_leaves_the_optimizer_untouched():
    import fused_densify as fd
    leaves, moments, action, noise = _case(R + 1, 15)
    opt = _optimizer(leaves, moments)
    before = [g["params"][0] for g in opt.param_groups]
    bad = action.clone()
    bad[R] = 4
    bad[3] = 255
    with pytest.raises(RuntimeError, match="2 action codes lie above 3"):
        fd.densify(opt, bad.to(DEV), noise=noise.to(DEV))
    assert all(a is b for a, b in zip(before, (g["params"][0] for g in opt.param_groups)))
    params, moms, steps = _state(opt)
    assert all(torch.equal(a, b) for a, b in zip(params, leaves)) and steps == [2] * 6
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(moms, moments))
    with pytest.raises(RuntimeError, match=r"S = \d+ split rows"):
        fd.densify(opt, action.to(DEV), noise=noise[1:].to(DEV))


def test_densify_and_prune_on_an_optimizer_equals_the_stock_sequence_and_steps_on():
    import fused_densify as fd
    P = 1000
    leaves, moments, grads = ref.make_case(P, rest=15, seed=P + 15)
    assert ref.margins(leaves, grads) >= 1e-3
    nan = grads.isnan().reshape(-1)
    accum, denom = torch.where(nan, torch.zeros(P), 4.0 * grads.reshape(-1)), torch.where(nan, torch.zeros(P), torch.full((P,), 4.0))
    assert torch.equal(torch.nan_to_num(accum / denom), torch.nan_to_num(grads.reshape(-1))) and bool((accum / denom).isnan().any())
    codes = fd.action_codes(leaves[ref.OPACITY], leaves[ref.SCALING], grads, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, ref.SCREEN)
    g = torch.nan_to_num(grads.reshape(-1), nan=0.0)
    stock_split = (g >= ref.MAX_GRAD) & (torch.exp(leaves[ref.SCALING]).max(dim=1).values > ref.PERCENT_DENSE * ref.EXTENT)
    S_stock = int(stock_split.sum())
    stock_noise = torch.randn(2 * S_stock, 3, generator=torch.Generator().manual_seed(9))
    kept = (codes == ref.SPLIT)[stock_split]
    noise = torch.cat([stock_noise[:S_stock][kept], stock_noise[S_stock:][kept]])
    want, want_moments = ref.stock_densify_and_prune(leaves, moments, grads, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, ref.SCREEN, stock_noise)
    opt = _optimizer(leaves, moments)
    stats = (accum.to(DEV), denom.to(DEV), torch.full((P,), 50.0, device=DEV))   # radii the reference never gets to test
    params, fresh, extras, (K, C, S) = fd.densify_and_prune(opt, stats, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, ref.SCREEN, noise=noise.to(DEV))
    Pout = K + C + 2 * S
    assert Pout == want[0].shape[0] and min(K, C, S) > 0 and extras == []
    assert all(t.shape == (Pout,) and t.device.type == "cuda" and not bool(t.any()) for t in fresh)
    got, got_moments, steps = _state(opt)
    assert steps == [2] * 6 and [params[n] for n in fd.LEAF_NAMES] == [grp["params"][0] for grp in opt.param_groups]
    first = K + C
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(a[:first], b[:first]), k
        if k not in (ref.XYZ, ref.SCALING):
            assert torch.equal(a, b), k
    scale = want[ref.XYZ][first:].double().norm(dim=1) + ref.expand(leaves, moments, codes, noise)["scale"]
    assert float(((got[ref.XYZ][first:].double() - want[ref.XYZ][first:].double()).norm(dim=1) / scale).max()) <= 1e-6
    assert float((got[ref.SCALING][first:].double() - want[ref.SCALING][first:].double()).abs().max()) <= 2e-6
    for k, (a, b) in enumerate(zip(got_moments, want_moments)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), k
    for p in params.values():
        assert p.requires_grad and p.shape[0] == Pout and p.is_leaf
        p.grad = torch.ones_like(p)
    opt.step()
    stepped, stepped_moments, steps = _state(opt)
    assert steps == [3] * 6 and all(m.shape[0] == Pout and v.shape[0] == Pout for m, v in stepped_moments)
    assert all(bool(torch.isfinite(s).all()) and not torch.equal(s, a) for s, a in zip(stepped, got))
    # use_max_radii2D hands the radii over: every row has been seen larger than the screen size
    opt = _optimizer(leaves, moments)
    _, _, _, counts = fd.densify_and_prune(opt, stats, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, ref.SCREEN, use_max_radii2D=True)
    assert counts == (0, 0, 0) and all(grp["params"][0].shape[0] == 0 for grp in opt.param_groups)


def test_prune_equals_mask_indexing():
    import fused_densify as fd
    leaves, moments, action, _ = _case(R + 1, 15)
    mask = action == ref.PRUNE
    opt = _optimizer(leaves, moments)
    extra = torch.arange(R + 1, dtype=torch.int32)
    params, extras, counts = fd.prune(opt, mask.to(DEV), extras=[(extra.to(DEV), False)])
    got, got_moments, steps = _state(opt)
    assert counts == (int((~mask).sum()), 0, 0) and steps == [2] * 6 and 0 < counts[0] < R + 1
    for a, (m, v), t, (wm, wv) in zip(got, got_moments, leaves, moments):
        assert torch.equal(a, t[~mask]) and torch.equal(m, wm[~mask]) and torch.equal(v, wv[~mask])
    assert torch.equal(extras[0].cpu(), extra[~mask])


def test_reset_opacity_caps_the_logits_and_zeroes_their_moments():
    import fused_densify as fd
    leaves, moments, _, _ = _case(R + 1, 15)
    opt = _optimizer(leaves, moments)
    p = fd.reset_opacity(opt)
    cap = math.log(0.01 / 0.99)
    got, got_moments, steps = _state(opt)
    assert p is opt.param_groups[3]["params"][0] and float(got[3].max()) <= cap and bool((leaves[3] > cap).any())
    assert torch.equal(got[3], leaves[3].clamp(max=cap)) and steps == [2] * 6
    assert not bool(got_moments[3][0].any()) and not bool(got_moments[3][1].any())
    for k in (0, 1, 2, 4, 5):
        assert torch.equal(got[k], leaves[k]) and torch.equal(got_moments[k][0], moments[k][0])
