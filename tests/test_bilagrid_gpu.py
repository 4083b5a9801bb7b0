"""GPU: the bilateral grid of affine colour transforms (include/gsr_bilagrid.h, fused_bilagrid.py) against tests/torch_bilagrid.py in
float64.

Slice shapes (H, W) / (L, GH, GW) against the 64x32 tile, the 64 KB node window and the gather's row segments: (7,9)/(2,2,2) smaller
than any tile with the minimal grid (gather in segments); (33,65)/(8,16,16) one-pixel remainder tiles in both directions and cells
about 4 px wide, so that one tile spans the whole node range and its window takes two passes; (70,130)/(3,2,5) interior tile seams
with cells larger than tiles; (5,6)/(3,9,11) more nodes than pixels; (4,5)/(40,3,60) a window of which not even two node rows fit
the LDS (the corners come from global memory).  Bars: out max|d| <= 1e-5; each gradient max|d| <= max(1e-5, 3 n32) max|g|, n32 the
same normalised error of the float32 evaluation of the reference against the float64 one (the rule of test_loss_ext_gpu.py).  The
inputs (torch_bilagrid.make_inputs) keep every luma coordinate 2e-3 away from an integer, so that fp32 and fp64 agree on every
cell; that is asserted on the CPU before anything is compared."""
import ctypes

import pytest
import torch

import torch_bilagrid as ref
import torch_loss_ext

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SLICE_SHAPES = (((7, 9), (2, 2, 2)), ((33, 65), (8, 16, 16)), ((70, 130), (3, 2, 5)), ((5, 6), (3, 9, 11)), ((4, 5), (40, 3, 60)))
TV_SHAPES = ((1, 12, 2, 2, 2), (3, 12, 8, 16, 16), (2, 12, 3, 2, 5), (12, 4, 3, 6))
_cache = {}


def _nerr(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / max(float(b.abs().max()), 1e-30))


def _case(hw, lgg):
    """-> inputs on the device, float64 reference, n32 per gradient; computed once and shared, never written to"""
    key = (hw, lgg)
    if key not in _cache:
        grid, image, go = ref.make_inputs(*hw, *lgg)
        ref.assert_inputs_are_safe(image, *lgg)
        out64, g64, affine64, inside = ref.slice_and_grads(grid, image, go)
        _, g32, _, _ = ref.slice_and_grads(grid, image, go, dtype=torch.float32)
        n32 = {n: _nerr(g32[n], g64[n]) for n in g64}
        _cache[key] = (grid.to(DEV), image.to(DEV), go.to(DEV), out64, g64, n32, affine64, inside)
    return _cache[key]


@pytest.mark.parametrize("hw,lgg", SLICE_SHAPES)
def test_slice_and_gradients_match_the_float64_reference(hw, lgg):
    import fused_bilagrid as fb
    grid, image, go, out64, g64, n32, affine64, inside = _case(hw, lgg)
    out, grads = fb.slice_and_grads(grid, image, go)
    err = float((out.double().cpu() - out64).abs().max())
    print(f"{hw} / {lgg}: out max|d| = {err:.2e}")
    for n in g64:
        print(f"{hw} / {lgg}: d/d{n}: n32 = {n32[n]:.2e} achieved = {_nerr(grads[n], g64[n]):.2e}")
    assert out.shape == out64.shape and bool(torch.isfinite(out).all()) and err <= 1e-5
    assert sorted(grads) == ["grid", "image"]
    for n in g64:
        assert grads[n].shape == g64[n].shape and bool(torch.isfinite(grads[n]).all()), n
        assert _nerr(grads[n], g64[n]) <= max(1e-5, 3.0 * n32[n]), (n, _nerr(grads[n], g64[n]), n32[n])
    # at a clamped pixel the guidance part is exactly zero: the affine part alone, within the bar
    clamped = ~inside
    assert bool(clamped.any())
    bar = max(1e-5, 3.0 * n32["image"]) * float(g64["image"].abs().max())
    assert float((grads["image"].double().cpu() - affine64)[:, clamped].abs().max()) <= bar


def test_unreached_nodes_get_a_positive_zero():
    import fused_bilagrid as fb
    grid, image, go, _, g64, *_ = _case((5, 6), (3, 9, 11))
    _, grads = fb.slice_and_grads(grid, image, go, want=("grid",))
    unreached = (g64["grid"] == 0)
    assert bool(unreached.any()) and bool((~unreached).any())
    got = grads["grid"].cpu()
    assert bool((got[unreached] == 0).all()) and not bool(torch.signbit(got[unreached]).any())


@pytest.mark.parametrize("hw,lgg", (((7, 9), (2, 2, 2)), ((33, 65), (8, 16, 16))))
def test_outputs_prefilled_with_nan_come_back_fully_written(hw, lgg):
    import fused_bilagrid as fb
    grid, image, go, *_ = _case(hw, lgg)
    (H, W), (L, GH, GW) = hw, lgg
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    out, dgrid, dimg = nan(3, H, W), nan(12, L, GH, GW), nan(3, H, W)
    lib = fb._lib()
    scratch = torch.full((lib.gsr_bilagrid_scratch_bytes(H, W, L, GH, GW),), 0xFF, dtype=torch.uint8, device=DEV)   # NaNs as floats
    a = fb.BilagridArgs(H=H, W=W, L=L, GH=GH, GW=GW, grid=grid.data_ptr(), img=image.data_ptr(), out=out.data_ptr(),
                        dL_dout=go.data_ptr(), dL_dgrid=dgrid.data_ptr(), dL_dimg=dimg.data_ptr(), scratch=scratch.data_ptr(),
                        stream=torch.cuda.current_stream(DEV).cuda_stream)
    fb._run("gsr_bilagrid_slice", ctypes.byref(a))
    fb._run("gsr_bilagrid_slice_backward", ctypes.byref(a))
    torch.cuda.synchronize()
    for t in (out, dgrid, dimg):
        assert bool(torch.isfinite(t).all())
    ref_out, ref_grads = fb.slice_and_grads(grid, image, go)
    assert torch.equal(out, ref_out) and torch.equal(dgrid, ref_grads["grid"]) and torch.equal(dimg, ref_grads["image"])


def test_only_the_gradients_asked_for_are_computed():
    import fused_bilagrid as fb
    grid, image, go, *_ = _case((70, 130), (3, 2, 5))
    _, both = fb.slice_and_grads(grid, image, go)
    calls = []
    real = fb._slice_backward_raw
    fb._slice_backward_raw = lambda *a: calls.append(real(*a)) or calls[-1]
    try:
        for name, need in (("grid", (True, False)), ("image", (False, True))):
            g, x = grid.clone().requires_grad_(need[0]), image.clone().requires_grad_(need[1])
            before = len(calls)
            fb.bilateral_grid_slice(g, x).backward(go)
            assert len(calls) == before + 1 and sorted(calls[-1]) == [name]
            got, other = (g.grad, x.grad) if name == "grid" else (x.grad, g.grad)
            assert other is None and torch.equal(got, both[name]), name
            _, raw = fb.slice_and_grads(grid, image, go, want=(name,))
            assert sorted(raw) == [name] and torch.equal(raw[name], both[name])
    finally:
        fb._slice_backward_raw = real
    g, x = grid.clone().requires_grad_(True), image.clone().requires_grad_(True)
    (2.0 * fb.bilateral_grid_slice(g, x)).backward(go)
    assert torch.equal(g.grad, fb.slice_and_grads(grid, image, 2.0 * go)[1]["grid"])
    assert torch.equal(x.grad, fb.slice_and_grads(grid, image, 2.0 * go)[1]["image"])


@pytest.mark.parametrize("hw,lgg", SLICE_SHAPES[:4])
def test_two_calls_give_the_same_bits(hw, lgg):
    import fused_bilagrid as fb
    grid, image, go, *_ = _case(hw, lgg)
    out_a, a = fb.slice_and_grads(grid, image, go)
    out_b, b = fb.slice_and_grads(grid, image, go)
    assert torch.equal(out_a, out_b) and torch.equal(a["grid"], b["grid"]) and torch.equal(a["image"], b["image"])


def test_the_identity_grid_leaves_the_image_as_it_is():
    import fused_bilagrid as fb
    _, image, *_ = _case((33, 65), (8, 16, 16))
    bg = fb.BilateralGrid(1).to(DEV)
    out = bg(image, 0)
    assert float((out.detach() - image).abs().max()) <= 1e-6


def test_a_slice_of_the_parameter_reaches_the_kernel_without_a_copy():
    import fused_bilagrid as fb
    _, image, go, *_ = _case((33, 65), (8, 16, 16))
    bg = fb.BilateralGrid(3, grid_X=5, grid_Y=3, grid_W=4).to(DEV)
    with torch.no_grad():
        bg.grids.add_(0.1 * torch.randn(bg.grids.shape, generator=torch.Generator().manual_seed(1)).to(DEV))
    seen = []
    real = fb._run

    def spy(name, *args):
        seen.append((name, args[0]._obj.grid))
        return real(name, *args)

    fb._run = spy
    try:
        bg(image, 1).backward(go)
    finally:
        fb._run = real
    where = bg.grids.data_ptr() + bg.grids[0].numel() * 4
    assert seen == [("gsr_bilagrid_slice", where), ("gsr_bilagrid_slice_backward", where)]
    grad = bg.grids.grad
    assert grad.shape == bg.grids.shape and bool((grad[0] == 0).all()) and bool((grad[2] == 0).all()) and bool((grad[1] != 0).any())
    assert torch.equal(grad[1], fb.slice_and_grads(bg.grids[1].detach(), image, go, want=("grid",))[1]["grid"])
    # a non-contiguous input is made contiguous
    g_t = bg.grids[1].detach().transpose(2, 3).contiguous().transpose(2, 3)
    assert not g_t.is_contiguous()
    assert torch.equal(fb.bilateral_grid_slice(g_t, image), fb.bilateral_grid_slice(bg.grids[1].detach(), image))


@pytest.mark.parametrize("shape", TV_SHAPES)
def test_total_variation_matches_the_float64_reference(shape):
    import fused_bilagrid as fb
    g = torch.Generator().manual_seed(3 + len(shape) + shape[-1])
    eye = torch.eye(3, 4, dtype=torch.float64).reshape(12, 1, 1, 1)
    grids = (eye + 0.2 * torch.randn(*shape, generator=g, dtype=torch.float64)).float()
    tv64, g64 = ref.tv_and_grad(grids)
    _, g32 = ref.tv_and_grad(grids, dtype=torch.float32)
    n32 = _nerr(g32, g64)
    x = grids.to(DEV).requires_grad_(True)
    tv = fb.total_variation_loss(x)
    (3.0 * tv).backward()
    val, raw = fb.tv_and_grad(x.detach())
    rel = abs(float(tv.detach()) - float(tv64)) / float(tv64)
    print(f"{shape}: tv = {float(tv.detach()):.8f} ref {float(tv64):.8f} rel {rel:.2e}; gradient n32 = {n32:.2e} achieved = {_nerr(raw, g64):.2e}")
    assert tv.dim() == 0 and rel <= 1e-6
    assert raw.shape == g64.shape and _nerr(raw, g64) <= max(1e-5, 3.0 * n32)
    assert float(val[0]) == float(tv.detach()) and torch.equal(x.grad, 3.0 * raw)   # a non-unit upstream gradient scales it
    val_b, raw_b = fb.tv_and_grad(x.detach())
    assert torch.equal(val, val_b) and torch.equal(raw, raw_b)
    val_c, none = fb.tv_and_grad(x.detach(), want_grad=False)
    assert none is None and torch.equal(val, val_c)
    assert not fb.total_variation_loss(x.detach()).requires_grad


def test_one_composed_step_follows_the_float64_reference():
    """slice -> training_loss, plus 10 tv, through FusedAdam: five iterations lower the loss, and every iterate stays within 1e-4 of
    the same steps done with the float64 reference and torch.optim.Adam(eps=1e-15).  gt keeps 0.05 from the image and the steps
    are 1e-3, so that no L1 sign changes on the way."""
    import fused_bilagrid as fb
    import fused_loss
    from fused_params import FusedAdam
    H, W, L, GH, GW = 33, 65, 4, 3, 5
    _, image, _ = ref.make_inputs(H, W, L, GH, GW)
    ref.assert_inputs_are_safe(image, L, GH, GW)
    g = torch.Generator().manual_seed(8)
    gt = (image.double() + torch.where(torch.rand(3, H, W, generator=g) < 0.5, -1.0, 1.0) * (0.05 + 0.15 * torch.rand(3, H, W, generator=g, dtype=torch.float64))).float()
    bg = fb.BilateralGrid(3, grid_X=GW, grid_Y=GH, grid_W=L).to(DEV)
    opt = FusedAdam([{"params": [bg.grids], "lr": 1e-3, "name": "bilagrid"}], lr=0.0, eps=1e-15)
    grids64 = bg.grids.detach().cpu().double().requires_grad_(True)
    opt64 = torch.optim.Adam([grids64], lr=1e-3, eps=1e-15)
    x, y = image.to(DEV), gt.to(DEV)
    losses = []
    for it in range(5):
        opt.zero_grad(set_to_none=True)
        loss = fused_loss.training_loss(fb.bilateral_grid_slice(bg.grids[1], x), y, 0.2) + 10 * bg.tv_loss()
        loss.backward()
        opt.step()
        opt64.zero_grad(set_to_none=True)
        loss64 = torch_loss_ext.loss_terms(ref.slice(grids64[1], image.double()), gt, 0.2)[0] + 10 * ref.total_variation(grids64)
        loss64.backward()
        opt64.step()
        d = float((bg.grids.detach().cpu().double() - grids64.detach()).abs().max())
        print(f"iteration {it}: loss {float(loss.detach()):.7f} ref {float(loss64.detach()):.7f}, iterate max|d| = {d:.2e}")
        assert abs(float(loss.detach()) - float(loss64.detach())) <= 1e-4 and d <= 1e-4, (it, float(loss.detach()), float(loss64.detach()), d)
        losses.append(float(loss.detach()))
    assert losses[4] < losses[0], losses
    assert float((bg.grids.detach()[1] - torch.eye(3, 4, device=DEV).reshape(12, 1, 1, 1)).abs().max()) > 1e-3
