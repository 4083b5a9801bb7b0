"""GPU: the extended fused loss (include/gsr_loss_ext.h, fused_loss.training_loss*) against tests/torch_loss_ext.py in float64.

Shapes against the 64x32 tile and the 11-tap window: (3,7,9) smaller than the window, (3,32,64) exactly one tile, (3,33,65) a
one-pixel remainder tile in both directions, (3,70,130) a middle tile with neighbours on both sides, (1,33,65) one channel.  Bars:
vals {loss, l1, ssim, depth_l1} within 1e-5, 1e-6, 1e-5, 1e-6; each gradient max|d| <= max(1e-5, 3 n32) max|g|, n32 the same
normalised error of the float32 evaluation of the reference against the float64 one (the rule of test_loss.py: E[x^2] - mu^2
cancels in fp32).  The inputs keep |x'' - y''| >= 1e-3 wherever the mask exceeds 0.05 and |d - d*| >= 1e-3 wherever the depth mask is
not 0, so that no L1 sign can differ between fp32 and fp64; that property is asserted on the CPU before anything is compared."""
import itertools

import pytest
import torch

import gsr_scene
import torch_loss_ext as ref
import util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAMBDA = 0.2
WEIGHT = 0.7
SHAPES_ALL = ((3, 7, 9), (3, 32, 64), (3, 70, 130), (1, 33, 65))
VAL_BARS = (1e-5, 1e-6, 1e-5, 1e-6)
_cache = {}


def _inputs(C, H, W, mask, exposure, depth, seed=11):
    """float32 CPU tensors of one case, built in float64 (the construction the module docstring describes)"""
    g = torch.Generator().manual_seed(seed + 1000 * C + 10 * H + W)
    rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = rand(C, H, W).float()
    kw = {}
    xp = x.double()
    if exposure:
        E = torch.cat([torch.eye(3, dtype=torch.float64) + 0.1 * randn(3, 3), 0.05 * randn(3, 1)], dim=1).float()
        kw["exposure"] = E
        Ed = E.double()
        xp = torch.stack([Ed[0, c] * xp[0] + Ed[1, c] * xp[1] + Ed[2, c] * xp[2] + Ed[c, 3] for c in range(3)])
    y = (xp + torch.where(rand(C, H, W) < 0.5, -1.0, 1.0) * (0.02 + 0.18 * rand(C, H, W))).float()
    c0 = 60 if W > 64 else W // 3                       # the zero columns straddle the tile seam at x = 64 where there is one
    c1 = min(W, c0 + 8) if W > 64 else max(c0 + 1, W // 2)
    m = torch.ones(H, W, dtype=torch.float64)
    if mask:
        m = 0.01 + 0.98 * rand(H, W)                   # values in (0, 1) ...
        m[: max(1, H // 3)] = 1.0                       # ... exactly 1 in the top rows ...
        m[H // 4:, c0:c1] = 0.0                         # ... and exactly 0 in a block of columns
        m = m.float()
        kw["mask"] = m
        assert (m == 0).any() and (m == 1).any() and ((m > 0) & (m < 1)).any()
        m = m.double()
    # no L1 sign can flip between fp32 and fp64
    gap = (m * xp - m * y.double()).abs()
    assert bool((gap[:, m > 0.05] >= 1e-3).all())
    if depth:
        d = (0.1 + 1.9 * rand(H, W)).float()
        dp = (d.double() + torch.where(rand(H, W) < 0.5, -1.0, 1.0) * (0.02 + 0.18 * rand(H, W))).float()
        k = (0.1 + 1.9 * rand(H, W))
        k[:, c0:c1] = 0.0
        k = k.float()
        assert (k == 0).any() and bool(((d.double() - dp.double()).abs()[k > 0] >= 1e-3).all())
        kw.update(invdepth=d.reshape(1, H, W), invdepth_prior=dp, invdepth_mask=k, invdepth_weight=WEIGHT)
    return x, y, kw


def _case(C, H, W, mask, exposure, depth):
    """-> (x, y, options on the device, float64 reference, n32 per gradient); computed once and shared, never written to"""
    key = (C, H, W, mask, exposure, depth)
    if key not in _cache:
        x, y, kw = _inputs(C, H, W, mask, exposure, depth)
        v64, g64 = ref.loss_and_grads(x, y, LAMBDA, dtype=torch.float64, **kw)
        _, g32 = ref.loss_and_grads(x, y, LAMBDA, dtype=torch.float32, **kw)
        n32 = {n: _nerr(g32[n], g64[n]) for n in g64}
        dev = {n: (t.to(DEV) if torch.is_tensor(t) else t) for n, t in kw.items()}
        _cache[key] = (x.to(DEV), y.to(DEV), dev, v64, g64, n32)
    return _cache[key]


def _nerr(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / max(float(b.abs().max()), 1e-30))


def _check_against_reference(got_vals, got_grads, v64, g64, n32, tag):
    for i, bar in enumerate(VAL_BARS):
        err = abs(float(got_vals[i]) - float(v64[i]))
        print(f"{tag} vals[{i}] = {float(got_vals[i]):.8f} ref {float(v64[i]):.8f} err {err:.2e} bar {bar:.0e}")
    for n in g64:
        print(f"{tag} d/d{n}: n32 = {n32[n]:.2e} achieved = {_nerr(got_grads[n], g64[n]):.2e}")
    for i, bar in enumerate(VAL_BARS):
        assert abs(float(got_vals[i]) - float(v64[i])) <= bar, (tag, i, float(got_vals[i]), float(v64[i]))
    assert set(got_grads) == set(g64), (tag, sorted(got_grads), sorted(g64))
    for n in g64:
        assert got_grads[n].shape == g64[n].shape and bool(torch.isfinite(got_grads[n]).all()), (tag, n)
        assert _nerr(got_grads[n], g64[n]) <= max(1e-5, 3.0 * n32[n]), (tag, n, _nerr(got_grads[n], g64[n]), n32[n])


SUBSETS = [(3, 33, 65) + s for s in itertools.product((False, True), repeat=3)]
OTHERS = [(C, H, W, True, C == 3, True) for C, H, W in SHAPES_ALL]


@pytest.mark.parametrize("C,H,W,mask,exposure,depth", SUBSETS + OTHERS)
def test_every_option_subset_matches_the_float64_reference(C, H, W, mask, exposure, depth):
    import fused_loss
    x, y, kw, v64, g64, n32 = _case(C, H, W, mask, exposure, depth)
    vals, grads = fused_loss.training_loss_and_grads(x, y, LAMBDA, **kw)
    _check_against_reference(vals.cpu(), grads, v64, g64, n32, f"({C},{H},{W}) m={mask:d} e={exposure:d} d={depth:d}")
    if not depth:
        assert float(vals[3]) == 0.0


def test_exact_zeros_under_the_masks_and_a_zero_weight():
    import fused_loss
    x, y, kw, *_ = _case(3, 70, 130, True, True, True)
    vals, grads = fused_loss.training_loss_and_grads(x, y, LAMBDA, **kw)
    zero = (kw["mask"] == 0)
    assert bool(zero.any()) and bool((grads["image"][:, zero] == 0).all())
    assert bool((grads["image"][:, kw["mask"] == 1] != 0).any())
    kz = (kw["invdepth_mask"] == 0)
    assert bool(kz.any()) and bool((grads["invdepth"][0][kz] == 0).all()) and bool((grads["invdepth"][0][~kz] != 0).all())
    vals0, grads0 = fused_loss.training_loss_and_grads(x, y, LAMBDA, **dict(kw, invdepth_weight=0.0))
    assert bool((grads0["invdepth"] == 0).all())
    plain = {n: t for n, t in kw.items() if not n.startswith("invdepth")}
    vals_plain, grads_plain = fused_loss.training_loss_and_grads(x, y, LAMBDA, **plain)
    assert float(vals0[0]) == float(vals_plain[0]) and float(vals0[3]) == float(vals[3]) > 0.0
    assert "invdepth" not in grads_plain


def test_neutral_options_agree_with_the_existing_loss():
    import fused_loss
    C, H, W = 3, 33, 65
    x, y, _, v64, g64, n32 = _case(C, H, W, False, False, False)
    E = torch.eye(3, 4, device=DEV)
    vals, grads = fused_loss.training_loss_and_grads(x, y, LAMBDA, mask=torch.ones(H, W, device=DEV), exposure=E)
    old_vals, old_grad = fused_loss.l1_ssim_loss_and_grad(x, y, LAMBDA)
    for i, bar in enumerate(VAL_BARS[:3]):
        assert abs(float(vals[i]) - float(old_vals[i])) <= bar, (i, float(vals[i]), float(old_vals[i]))
    bar = max(1e-5, 3.0 * n32["image"])
    print(f"neutral: against l1_ssim_loss_and_grad {_nerr(grads['image'], old_grad):.2e}, bar {bar:.2e}")
    assert _nerr(grads["image"], old_grad) <= bar
    assert _nerr(grads["image"], g64["image"]) <= bar
    # dL/dexposure at the identity, against the reference's
    _, r64 = ref.loss_and_grads(x.cpu(), y.cpu(), LAMBDA, exposure=E.cpu(), dtype=torch.float64)
    _, r32 = ref.loss_and_grads(x.cpu(), y.cpu(), LAMBDA, exposure=E.cpu(), dtype=torch.float32)
    nE = _nerr(r32["exposure"], r64["exposure"])
    print(f"neutral: d/dexposure n32 = {nE:.2e} achieved = {_nerr(grads['exposure'], r64['exposure']):.2e}")
    assert _nerr(grads["exposure"], r64["exposure"]) <= max(1e-5, 3.0 * nE)


def test_two_calls_give_the_same_bits():
    import fused_loss
    x, y, kw, *_ = _case(3, 70, 130, True, True, True)
    a_vals, a = fused_loss.training_loss_and_grads(x, y, LAMBDA, **kw)
    b_vals, b = fused_loss.training_loss_and_grads(x, y, LAMBDA, **kw)
    assert torch.equal(a_vals, b_vals)
    assert sorted(a) == sorted(b) == ["exposure", "image", "invdepth"]
    for n in a:
        assert torch.equal(a[n], b[n]), n


def test_autograd_plumbing_is_exact():
    import fused_loss
    from diff_gaussian_rasterization import GaussianRasterizer
    W, H = 64, 48
    scene, cam = gsr_scene.make_scene(200, -3.0, sh_degree=1, seed=4), gsr_scene.make_camera(W, H)
    st = util.hip_settings(scene, cam, 1, DEV)
    g = torch.Generator().manual_seed(9)
    gt = torch.rand(3, H, W, generator=g).to(DEV)
    mask = (torch.rand(H, W, generator=g) > 0.2).to(DEV)      # a bool mask: converted by the Python layer
    prior = torch.rand(H, W, generator=g).to(DEV)
    dmask = torch.rand(H, W, generator=g).to(DEV)
    E0 = (torch.eye(3, 4) + 0.05 * torch.randn(3, 4, generator=g)).to(DEV)
    names = ("means3D", "means2D", "shs", "opacities", "scales", "rotations")

    def render():
        t = {"means3D": scene.means3D.to(DEV).clone().requires_grad_(True),
             "means2D": torch.zeros(scene.means3D.shape, device=DEV, requires_grad=True),
             "shs": scene.shs.to(DEV).clone().requires_grad_(True), "opacities": scene.opacities.to(DEV).clone().requires_grad_(True),
             "scales": scene.scales.to(DEV).clone().requires_grad_(True), "rotations": scene.rotations.to(DEV).clone().requires_grad_(True)}
        color, _, invdepth, _ = GaussianRasterizer(st, depth_alpha="invdepth")(**t)
        return t, color, invdepth

    opts = dict(mask=mask, invdepth_prior=prior, invdepth_mask=dmask, invdepth_weight=WEIGHT)
    t1, color, invdepth = render()
    E = E0.clone().requires_grad_(True)
    loss = fused_loss.training_loss(color, gt, LAMBDA, exposure=E, invdepth=invdepth, **opts)
    (3.0 * loss).backward()

    t2, color2, invdepth2 = render()
    assert torch.equal(color, color2) and torch.equal(invdepth, invdepth2)
    vals, raw = fused_loss.training_loss_and_grads(color2, gt, LAMBDA, exposure=E0, invdepth=invdepth2, **opts)
    assert raw["invdepth"].shape == invdepth2.shape and float(vals[0]) == float(loss.detach())
    torch.autograd.backward([color2, invdepth2], [3.0 * raw["image"], 3.0 * raw["invdepth"]])
    for n in names:
        assert t1[n].grad is not None and torch.equal(t1[n].grad, t2[n].grad), n
    assert any(float(t1[n].grad.abs().max()) > 0 for n in names)
    assert E.grad.shape == (3, 4) and torch.equal(E.grad, 3.0 * raw["exposure"])

    # no gradient is computed for an input that does not require one
    calls = []
    real = fused_loss.training_loss_and_grads
    fused_loss.training_loss_and_grads = lambda *a, **k: calls.append(real(*a, **k)) or calls[-1]
    try:
        E2 = E0.clone().requires_grad_(True)
        fused_loss.training_loss(color.detach(), gt, LAMBDA, exposure=E2, invdepth=invdepth.detach(), **opts).backward()
    finally:
        fused_loss.training_loss_and_grads = real
    assert len(calls) == 1 and sorted(calls[0][1]) == ["exposure"]
    assert torch.equal(E2.grad, raw["exposure"])


def test_full_size_against_stock_pytorch_in_fp32():
    import fused_loss
    C, H, W = 3, 1080, 1980
    g = torch.Generator().manual_seed(3)
    x = torch.rand(C, H, W, generator=g).to(DEV)
    mask = torch.rand(H, W, generator=g).to(DEV)
    mask[:, 600:700] = 0.0
    E = (torch.eye(3, 4) + 0.05 * torch.randn(3, 4, generator=g)).to(DEV)
    # gt and the prior keep their distance from x' and d, as in the small cases: two fp32 evaluations must agree on every L1 sign
    Ed, xd = E.double(), x.double()
    xp = torch.stack([Ed[0, c] * xd[0] + Ed[1, c] * xd[1] + Ed[2, c] * xd[2] + Ed[c, 3] for c in range(3)])
    off = lambda *s: (torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0) * (0.02 + 0.18 * torch.rand(*s, generator=g))).to(DEV)
    gt = (xp + off(C, H, W)).float()
    d = torch.rand(H, W, generator=g).to(DEV)
    dp = (d.double() + off(H, W)).float()
    dk = torch.rand(H, W, generator=g).to(DEV)
    assert float((xp - gt.double()).abs().min()) >= 1e-3 and float((d.double() - dp.double()).abs().min()) >= 1e-3
    kw = dict(mask=mask, exposure=E, invdepth=d, invdepth_prior=dp, invdepth_mask=dk, invdepth_weight=WEIGHT)
    vals, grads = fused_loss.training_loss_and_grads(x, gt, LAMBDA, **kw)
    rvals, rgrads = ref.loss_and_grads(x, gt, LAMBDA, dtype=torch.float32, **kw)
    assert bool(torch.isfinite(vals).all()) and all(bool(torch.isfinite(t).all()) for t in grads.values())
    assert abs(float(vals[0]) - float(rvals[0])) < 1e-5, (float(vals[0]), float(rvals[0]))
    for n in ("image", "exposure", "invdepth"):
        err, top = float((grads[n] - rgrads[n]).abs().max()), float(rgrads[n].abs().max())
        print(f"full size d/d{n}: max|d| = {err:.3e}, max|g| = {top:.3e}")
        assert err <= 2e-3 * top, (n, err, top)
