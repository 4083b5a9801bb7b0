"""GPU: the fused neighbour-rigidity losses (include/gsr_rigidity.h, fused_rigidity.py) against tests/torch_rigidity.py in float64 on
the same inputs (the tables go in through from_tables, so both sides read the same numbers).

Values: the relative error of each of total / rigid / rot / iso is at most max(2 e_stock, b).  e_stock is the error of the stock
float32 sequence (tests/torch_rigidity.py (a) in float32, evaluated here on the CPU) on the same inputs.  b counts the roundings on the
way to a value, each at most 2^-24 of a sum of positive terms: 48 on the longest chain of one edge's term (rigid: the norm of r 8 and
the division 1, a component of q (x) p 7, the norm of rel 8 and the division 1, an entry of R 5, a component of R^T c with its
difference c 6, minus o 1, the squared norm 5, times w, plus 1e-20, the square root 3; 45, rounded up), ceil(K / LANES) additions in
a lane, log2(256) = 8 levels of the workgroup's tree, and 4 for the float64 fold, the division by N_e and the final rounding:
b = (48 + ceil(K / LANES) + 8 + 4) 2^-24.  Cancellation in R^T c - o, rel_j - rel_i and |c| - d can amplify a rounding beyond its
count; that is what the e_stock branch is for.
Gradients: per row |g - g64| / S_j <= 2 e_stock + 2^-22 (the convention of test_mcmc_gpu.py), |.| the Euclidean norm of the row's
difference, S_j the float64 sum of the norms of every contribution added into row j (torch_rigidity.analytic_grads), e_stock the
largest such figure of the stock float32 autograd sequence over the rows.
A table without an edge (P = 1) gives exactly 0 everywhere."""
import math

import pytest
import torch

import torch_rigidity as tr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("idx", "prev_offset", "prev_dist", "weight", "prev_inv_rot")
_cache = {}


def _side(P):
    return tr.SIDES.get(P, 0.02)   # P = 1, 2: close enough for a weight that says something


def _tables(kind, P, K):
    xyz0, rot0 = tr.make_cloud(P, side=_side(P))
    mask = None
    if kind == "mask":   # whole rows of -1: what the tables hold there is never read
        mask = torch.rand(P, generator=torch.Generator().manual_seed(P)) < 0.7
    t = tr.capture(xyz0, rot0, K, mask=mask)
    if kind == "mask":
        for name in ("prev_offset", "prev_dist", "weight"):
            t[name][~mask] = float("nan")
    if kind == "star":   # the first column names row 0 everywhere: P edges on one target, the longest list of the per-point sum
        off = xyz0[0] - xyz0
        d2 = (off * off).sum(-1)
        t["idx"][:, 0] = 0
        t["prev_offset"][:, 0], t["prev_dist"][:, 0], t["weight"][:, 0] = off, torch.sqrt(d2), torch.exp(-200.0 * d2)
    return xyz0, rot0, t, mask


def _case(kind, P, K, lambdas=tr.LAMBDAS, perturbed=True):
    """the leaves, the tables, the float64 reference and the stock float32 sequence's errors; computed once, shared, never written to"""
    key = (kind, P, K, lambdas, perturbed)
    if key not in _cache:
        xyz0, rot0, t, mask = _tables(kind, P, K)
        xyz, rot = tr.perturb(xyz0, rot0, _side(P)) if perturbed else (xyz0, rot0)
        v64, gx64, gr64 = tr.loss_and_grads(xyz, rot, t, lambdas)
        _, _, Sx, Sr = tr.analytic_grads(xyz, rot, t, lambdas)
        v32, gx32, gr32 = tr.loss_and_grads(xyz, rot, t, lambdas, dtype=torch.float32)
        e_val = torch.where(v64 != 0, (v32.double() - v64).abs() / v64.abs().clamp(min=1e-300), torch.zeros_like(v64))
        _cache[key] = dict(xyz=xyz, rot=rot, t=t, mask=mask, v64=v64, gx64=gx64, gr64=gr64, Sx=Sx, Sr=Sr, e_val=e_val,
                           e_gx=float(tr.row_error(gx32, gx64, Sx).max()), e_gr=float(tr.row_error(gr32, gr64, Sr).max()))
    return _cache[key]


def _state(c):
    import fused_rigidity as fr
    return fr.RigidityState.from_tables(*(c["t"][n].to(DEV) for n in NAMES), c["xyz"].shape[0])


def _check_against_reference(c, values, gx, gr, K, lambdas=tr.LAMBDAS):
    import fused_rigidity as fr
    b = (48 + math.ceil(K / fr.LANES) + 8 + 4) * 2.0 ** -24
    v = values.double().cpu()
    assert bool(torch.isfinite(v).all())
    for k, name in enumerate(("total", "rigid", "rot", "iso")):
        want, stock = float(c["v64"][k]), float(c["e_val"][k])
        if want == 0.0:
            assert float(v[k]) == 0.0, name
            continue
        rel = abs(float(v[k]) - want) / abs(want)
        print(f"  {name}: {float(v[k]):.9e} (float64 {want:.9e}); relative error {rel:.2e}, stock float32 {stock:.2e}, bar {max(2 * stock, b):.2e}")
        assert rel <= max(2 * stock, b), (name, rel, stock, b)
    for name, g, g64, S, stock in (("xyz", gx, c["gx64"], c["Sx"], c["e_gx"]), ("rotation", gr, c["gr64"], c["Sr"], c["e_gr"])):
        assert bool(torch.isfinite(g).all())
        achieved = float(tr.row_error(g.cpu(), g64, S).max())
        print(f"  d/d{name}: worst row error / S_j {achieved:.2e}, stock float32 {stock:.2e}, bar {2 * stock + 2.0 ** -22:.2e}; max |g| {float(g64.abs().max()):.3e}")
        assert achieved <= 2 * stock + 2.0 ** -22, (name, achieved, stock)


CASES = [("knn", 1, 20), ("knn", 2, 20), ("knn", 63, 20), ("knn", 257, 20), ("knn", 1000, 20), ("knn", 4097, 16),   # a lone lane ... several workgroups
         ("knn", 257, 1), ("knn", 257, 3), ("knn", 257, 32), ("knn", 63, 32),
         ("star", 257, 20), ("mask", 1000, 20)]


@pytest.mark.parametrize("kind,P,K", CASES)
def test_values_and_gradients_match_the_float64_reference(kind, P, K):
    import fused_rigidity as fr
    c = _case(kind, P, K)
    state = _state(c)
    valid = c["t"]["idx"] >= 0
    assert state.num_edges == int(valid.sum()) and state.K == K and state.num_points == P
    print(f"{kind}, P = {P}, K = {K}, N_e = {state.num_edges}:")
    values, grads = fr.rigidity_loss_and_grads(c["xyz"].to(DEV), c["rot"].to(DEV), state)
    _check_against_reference(c, values, grads["xyz"], grads["rotation"], K)
    if P == 2:
        assert bool((~valid[:, 1:]).all()) and bool(valid[:, 0].all())   # fewer points than K: every row has -1 places
    if P == 1:
        assert state.num_edges == 0 and bool((values == 0).all()) and bool((grads["xyz"] == 0).all()) and bool((grads["rotation"] == 0).all())
    if kind == "star":
        assert int((c["t"]["idx"] == 0).sum()) >= P   # the fold list of row 0
    if kind == "mask":   # rows without an edge in or out: exactly 0, whatever their table rows hold
        out = ~c["mask"]
        assert int(out.sum()) > 100 and bool(torch.isnan(c["t"]["weight"][out]).all())
        assert bool((grads["xyz"].cpu()[out] == 0).all()) and bool((grads["rotation"].cpu()[out] == 0).all())
        assert bool((grads["xyz"].cpu()[c["mask"]] != 0).any())


@pytest.mark.parametrize("lambdas", ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)))
def test_a_single_weight_reproduces_its_term_alone(lambdas):
    import fused_rigidity as fr
    P, K = 257, 20
    c = _case("knn", P, K, lambdas)
    state = _state(c)
    x, r = c["xyz"].to(DEV), c["rot"].to(DEV)
    print(f"lambdas = {lambdas}:")
    values, grads = fr.rigidity_loss_and_grads(x, r, state, *lambdas)
    _check_against_reference(c, values, grads["xyz"], grads["rotation"], K, lambdas)
    both, _ = fr.rigidity_loss_and_grads(x, r, state)
    k = 1 + lambdas.index(1.0)
    assert torch.equal(values[1:], both[1:]) and float(values[0]) == float(both[k])   # the terms do not depend on the weights
    if lambdas[0] == 0.0 and lambdas[1] == 0.0:
        assert bool((grads["rotation"] == 0).all())   # the isometry term does not see the rotations


def test_determinism_routing_and_the_terms():
    import fused_rigidity as fr
    c = _case("knn", 1000, 20)
    state = _state(c)
    x, r = c["xyz"].to(DEV), c["rot"].to(DEV)
    values, grads = fr.rigidity_loss_and_grads(x, r, state)
    again, grads2 = fr.rigidity_loss_and_grads(x, r, state)
    assert torch.equal(values, again) and torch.equal(grads["xyz"], grads2["xyz"]) and torch.equal(grads["rotation"], grads2["rotation"])
    vx, only_x = fr.rigidity_loss_and_grads(x, r, state, want=("xyz",))
    vr, only_r = fr.rigidity_loss_and_grads(x, r, state, want=("rotation",))
    assert set(only_x) == {"xyz"} and set(only_r) == {"rotation"}
    assert torch.equal(only_x["xyz"], grads["xyz"]) and torch.equal(only_r["rotation"], grads["rotation"])
    assert torch.equal(vx, values) and torch.equal(vr, values)
    v0, none = fr.rigidity_loss_and_grads(x, r, state, want=())   # the value-only pass is another instantiation: the reference's bar, not the bits
    assert none == {}
    b = (48 + math.ceil(20 / fr.LANES) + 8 + 4) * 2.0 ** -24
    for k in range(4):
        assert abs(float(v0[k]) - float(c["v64"][k])) / float(c["v64"][k]) <= max(2 * float(c["e_val"][k]), b)
    total, terms = float(values[0]), values[1:].double().cpu()
    assert abs(total - float(4.0 * terms[0] + 4.0 * terms[1] + 2.0 * terms[2])) <= 2.0 ** -23 * total   # within one rounding
    half, _ = fr.rigidity_loss_and_grads(x, r, state, 0.5, 0.25, 3.0, want=())
    assert abs(float(half[0]) - float(0.5 * terms[0] + 0.25 * terms[1] + 3.0 * terms[2])) <= 2.0 ** -23 * float(half[0])


def test_autograd_scales_the_raw_gradients_and_takes_strided_leaves():
    import fused_rigidity as fr
    c = _case("knn", 1000, 20)
    P = 1000
    state = _state(c)
    values, raw = fr.rigidity_loss_and_grads(c["xyz"].to(DEV), c["rot"].to(DEV), state)
    # strided views of larger leaves
    big_x = torch.zeros((P, 5), device=DEV)
    big_x[:, 1:4] = c["xyz"].to(DEV)
    big_r = torch.zeros((2 * P, 4), device=DEV)
    big_r[::2] = c["rot"].to(DEV)
    big_x.requires_grad_(True)
    big_r.requires_grad_(True)
    x, r = big_x[:, 1:4], big_r[::2]
    assert not x.is_contiguous() and not r.is_contiguous()
    v_s, raw_s = fr.rigidity_loss_and_grads(x, r, state)
    assert torch.equal(v_s, values) and torch.equal(raw_s["xyz"], raw["xyz"]) and torch.equal(raw_s["rotation"], raw["rotation"])
    loss = fr.rigidity_loss(x, r, state)
    assert loss.dim() == 0 and loss.requires_grad and float(loss.detach()) == float(values[0])
    (3.0 * loss).backward()
    assert torch.equal(big_x.grad[:, 1:4], 3.0 * raw["xyz"]) and torch.equal(big_r.grad[::2], 3.0 * raw["rotation"])
    assert bool((big_x.grad[:, 0] == 0).all()) and bool((big_r.grad[1::2] == 0).all())
    # only what needs a gradient gets one
    xl = c["xyz"].to(DEV).requires_grad_(True)
    rl = c["rot"].to(DEV).requires_grad_(True)
    (g_x,) = torch.autograd.grad(fr.rigidity_loss(xl, rl.detach(), state), xl)
    (g_r,) = torch.autograd.grad(fr.rigidity_loss(xl.detach(), rl, state), rl)
    assert torch.equal(g_x, raw["xyz"]) and torch.equal(g_r, raw["rotation"])
    assert not fr.rigidity_loss(xl.detach(), rl.detach(), state).requires_grad
    # the terms for logging
    loss, rigid, rot, iso = fr.rigidity_loss_terms(xl, rl, state)
    assert loss.requires_grad and not (rigid.requires_grad or rot.requires_grad or iso.requires_grad)
    assert float(loss.detach()) == float(values[0]) and [float(rigid), float(rot), float(iso)] == values[1:].tolist()
    loss.backward()
    assert torch.equal(xl.grad, raw["xyz"]) and torch.equal(rl.grad, raw["rotation"])


def test_an_unperturbed_state_is_finite():
    """current = captured: the differences are rounding noise under a square root, and so is the gradient in any float32 evaluation;
    nothing is compared, everything is finite"""
    import fused_rigidity as fr
    c = _case("knn", 1000, 20, perturbed=False)
    values, grads = fr.rigidity_loss_and_grads(c["xyz"].to(DEV), c["rot"].to(DEV), _state(c))
    assert bool(torch.isfinite(values).all()) and bool(torch.isfinite(grads["xyz"]).all()) and bool(torch.isfinite(grads["rotation"]).all())
    assert bool((values[1:] >= 0).all())


def test_capture_on_the_device_builds_the_reference_tables():
    import fused_rigidity as fr
    P, K = 1000, 20
    xyz0, rot0 = tr.make_cloud(P)
    for mask in (None, torch.rand(P, generator=torch.Generator().manual_seed(9)) < 0.6):
        want = tr.capture(xyz0, rot0, K, mask=mask)
        x = xyz0.to(DEV).requires_grad_(True)
        state = fr.RigidityState.capture(x, rot0.to(DEV), K, mask=None if mask is None else mask.to(DEV))
        assert torch.equal(state.idx.cpu(), want["idx"]) and torch.equal(state.prev_offset.cpu(), want["prev_offset"])
        assert torch.allclose(state.prev_dist.cpu(), want["prev_dist"], rtol=2.0 ** -22, atol=0)
        assert torch.allclose(state.weight.cpu(), want["weight"], rtol=2.0 ** -20, atol=1e-40)   # two implementations of exp
        assert float((state.prev_inv_rot.cpu() - want["prev_inv_rot"]).abs().max()) <= 2.0 ** -22
        assert state.num_edges == int((want["idx"] >= 0).sum()) and state.num_points == P and state.K == K
        assert not any(t.requires_grad for t in (state.prev_offset, state.prev_dist, state.weight, state.prev_inv_rot))
        if mask is not None:
            assert bool((state.idx.cpu()[~mask] == -1).all())
            xyz, rot = tr.perturb(xyz0, rot0, tr.SIDES[P])
            _, grads = fr.rigidity_loss_and_grads(xyz.to(DEV), rot.to(DEV), state)
            assert bool((grads["xyz"].cpu()[~mask] == 0).all()) and bool((grads["rotation"].cpu()[~mask] == 0).all())
    # no point at all
    empty = fr.RigidityState.capture(torch.zeros((0, 3), device=DEV), torch.zeros((0, 4), device=DEV), K)
    values, grads = fr.rigidity_loss_and_grads(torch.zeros((0, 3), device=DEV), torch.zeros((0, 4), device=DEV), empty)
    assert empty.num_edges == 0 and bool((values == 0).all()) and grads["xyz"].shape == (0, 3) and grads["rotation"].shape == (0, 4)
