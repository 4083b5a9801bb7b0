"""GPU: the default training loss (csrc/loss.hip, fused_loss.l1_ssim_loss*) against tests/torch_loss_ext.py in float64; without an
option that reference is the plain loss.  loss.hip keeps its own forward, backward and fold kernels, so it gets the shapes the
extended loss got, against the 64x32 tile and the 11-tap window, and more: C other than 3, W below one float4 quad, and more tile
partials than the fold has threads.

Bars: vals {loss, l1, ssim} within 1e-5, 1e-6, 1e-5 of float64; gradient max|d| <= max(1e-5, 3 n32) max|g|, n32 the same normalised
error of the float32 evaluation of the reference against the float64 one (the rule of test_loss.py).  The inputs are those of
test_loss_ext_gpu._inputs without options: they keep |x - y| >= 1e-3 everywhere, so that no L1 sign can differ between fp32 and
fp64; asserted on the CPU before anything is compared."""
import numpy as np
import pytest
import torch

import torch_loss_ext as ref
from test_loss_ext_gpu import _inputs, _nerr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAMBDA = 0.2
VAL_BARS = (1e-5, 1e-6, 1e-5)
TILE_X, TILE_Y, FOLD_THREADS = 64, 32, 256      # csrc/gsr_loss_tile.h, gsr_loss_finalize_kernel
SHAPES = ((3, 7, 9),        # smaller than the window
          (3, 32, 64),      # exactly one tile
          (3, 33, 65),      # one-pixel remainder tiles both ways
          (3, 70, 130),     # a middle tile
          (1, 33, 65),      # one channel
          (3, 5, 200),      # H below the window, four tiles across
          (2, 100, 3),      # W below one float4 quad, C = 2
          (4, 11, 11),      # C = 4
          (3, 321, 577))    # 330 partials, past the fold's 256 threads
_cache = {}


def _partials(C, H, W):
    return -(-W // TILE_X) * -(-H // TILE_Y) * C


def _case(C, H, W, kink=False):
    """-> (x, y on the device, float64 vals, float64 gradient, n32); computed once and shared, never written to"""
    key = (C, H, W, kink)
    if key not in _cache:
        x, y, kw = _inputs(C, H, W, False, False, False)
        assert kw == {}
        if kink:      # a bit-equal block that straddles the tile seam at x = 64: there the L1 term has no gradient
            y = y.clone()
            y[:, 10:20, 60:68] = x[:, 10:20, 60:68]
        gap = (x.double() - y.double()).abs()
        assert bool(((gap >= 1e-3) | (x == y)).all()) and bool((x == y).any()) == kink
        v64, g64 = ref.loss_and_grads(x, y, LAMBDA, dtype=torch.float64)
        _, g32 = ref.loss_and_grads(x, y, LAMBDA, dtype=torch.float32)
        assert sorted(g64) == ["image"] and float(v64[3]) == 0.0
        _cache[key] = (x.to(DEV), y.to(DEV), v64, g64["image"], _nerr(g32["image"], g64["image"]))
    return _cache[key]


def _check(tag, vals, grad, v64, g64, n32):
    ach, bar = _nerr(grad, g64), max(1e-5, 3.0 * n32)
    for i, vb in enumerate(VAL_BARS):
        print(f"{tag} vals[{i}] = {float(vals[i]):.8f} ref {float(v64[i]):.8f} err {abs(float(vals[i]) - float(v64[i])):.2e} bar {vb:.0e}")
    print(f"{tag} d/dimage: n32 = {n32:.2e} achieved = {ach:.2e} bar = {bar:.2e}")
    for i, vb in enumerate(VAL_BARS):
        assert abs(float(vals[i]) - float(v64[i])) <= vb, (tag, i, float(vals[i]), float(v64[i]))
    assert grad.shape == g64.shape and grad.dtype == torch.float32 and grad.is_contiguous()
    assert bool(torch.isfinite(grad).all()) and ach <= bar, (tag, ach, bar)


@pytest.mark.parametrize("C,H,W", SHAPES)
def test_every_tile_and_window_edge_matches_the_float64_reference(C, H, W):
    import fused_loss
    if (C, H, W) == SHAPES[-1]:
        assert _partials(C, H, W) == 330 > FOLD_THREADS      # the fold's strided loop takes a second round
    else:
        assert _partials(C, H, W) <= FOLD_THREADS
    x, y, v64, g64, n32 = _case(C, H, W)
    vals, grad = fused_loss.l1_ssim_loss_and_grad(x, y, LAMBDA)
    assert vals.shape == (3,)
    _check(f"({C},{H},{W})", vals.cpu(), grad, v64, g64, n32)


def test_the_l1_kink_on_a_tile_seam():
    """where x == y bit for bit the gradient is the SSIM part alone"""
    import fused_loss
    C, H, W = 3, 70, 130
    x, y, v64, g64, n32 = _case(C, H, W, kink=True)
    vals, grad = fused_loss.l1_ssim_loss_and_grad(x, y, LAMBDA)
    _check("kink (3,70,130)", vals.cpu(), grad, v64, g64, n32)
    eq = (x == y)
    assert int(eq.sum()) == 3 * 10 * 8
    # inside the block the reference has no L1 part (|.|' = 0 at 0), and the block on its own is held to the same bar
    assert float((grad[eq].double().cpu() - g64[eq.cpu()]).abs().max()) <= max(1e-5, 3.0 * n32) * float(g64.abs().max())


def test_views_and_other_dtypes_give_the_bits_of_the_contiguous_float32_copy():
    import fused_loss
    C, H, W = 3, 33, 65
    x, y, *_ = _case(C, H, W)
    vals0, grad0 = fused_loss.l1_ssim_loss_and_grad(x, y, LAMBDA)
    hwc = x.permute(1, 2, 0).contiguous()                    # the image as (H, W, C) memory
    big = torch.rand(5, H, W, generator=torch.Generator().manual_seed(1)).to(DEV)
    big[1:4] = x
    wide = torch.rand(C, H, W + 7, generator=torch.Generator().manual_seed(2)).to(DEV)
    wide[:, :, 3:3 + W] = x
    ywide = torch.rand(C, H, 2 * W, generator=torch.Generator().manual_seed(3)).to(DEV)
    ywide[:, :, ::2] = y
    layouts = {"permuted image": (hwc.permute(2, 0, 1), y), "channel slice": (big[1:4], y), "column crop": (wide[:, :, 3:3 + W], y),
               "float64 gt": (x, y.double()), "strided gt": (x, ywide[:, :, ::2])}
    for tag, (a, b) in layouts.items():
        assert torch.equal(a, x) and torch.equal(b.float(), y)
        if tag == "channel slice":
            assert a.is_contiguous() and a.data_ptr() != big.data_ptr()
        elif "gt" not in tag:
            assert not a.is_contiguous()
        if tag == "strided gt":
            assert not b.is_contiguous()
        vals, grad = fused_loss.l1_ssim_loss_and_grad(a, b, LAMBDA)
        assert torch.equal(vals, vals0) and torch.equal(grad, grad0), tag
        assert grad.shape == (C, H, W) and grad.is_contiguous(), tag
    # and through autograd: the gradient arrives in the layout of the leaf
    leaf = hwc.clone().requires_grad_(True)
    fused_loss.l1_ssim_loss(leaf.permute(2, 0, 1), y, LAMBDA).backward()
    assert leaf.grad.shape == (H, W, C) and torch.equal(leaf.grad.permute(2, 0, 1), grad0)


def test_autograd_plumbing_is_exact():
    import fused_loss
    x, y, *_ = _case(3, 33, 65)
    vals0, raw = fused_loss.l1_ssim_loss_and_grad(x, y, LAMBDA)
    img = x.clone().requires_grad_(True)
    loss, l1, ssim = fused_loss.l1_ssim_loss_terms(img, y, LAMBDA)
    assert torch.equal(torch.stack((loss.detach(), l1, ssim)), vals0) and not l1.requires_grad and not ssim.requires_grad
    (3.0 * loss).backward()
    assert torch.equal(img.grad, 3.0 * raw)
    # an image that requires no gradient: the same values, and no gradient is computed
    vals1, none = fused_loss.l1_ssim_loss_and_grad(x, y, LAMBDA, want_grad=False)
    assert none is None and torch.equal(vals1, vals0)
    calls = []
    real = fused_loss.l1_ssim_loss_and_grad
    fused_loss.l1_ssim_loss_and_grad = lambda *a, **k: calls.append(real(*a, **k)) or calls[-1]
    try:
        terms = fused_loss.l1_ssim_loss_terms(x, y, LAMBDA)
    finally:
        fused_loss.l1_ssim_loss_and_grad = real
    assert len(calls) == 1 and calls[0][1] is None
    assert not terms[0].requires_grad and torch.equal(torch.stack(terms), vals0)


@pytest.mark.parametrize("C,H,W", [(3, 33, 65), (2, 100, 3)])
def test_every_output_element_is_written_and_nothing_beside_it(C, H, W):
    """gsr_l1_ssim_loss with vals and the gradient prefilled with NaN, the gradient inside a larger NaN buffer: every element comes
    back finite with the bits of the Python layer's call, and the guard elements are still NaN"""
    import fused_loss
    x, y, *_ = _case(C, H, W)
    vals0, grad0 = fused_loss.l1_ssim_loss_and_grad(x, y, LAMBDA)
    L = fused_loss._lib()
    n = C * H * W
    pad = 4 + (-n) % 4
    vals = torch.full((3 + 5,), float("nan"), device=DEV)
    buf = torch.full((4 + n + pad,), float("nan"), device=DEV)
    scratch = torch.empty(L.gsr_loss_scratch_bytes(C, H, W), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    rc = L.gsr_l1_ssim_loss(C, H, W, x.data_ptr(), y.data_ptr(), LAMBDA, vals.data_ptr(), buf.data_ptr() + 16, scratch.data_ptr(),
                            torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isfinite(vals[:3]).all()) and bool(torch.isnan(vals[3:]).all()) and torch.equal(vals[:3], vals0)
    grad = buf[4:4 + n].view(C, H, W)
    assert bool(torch.isfinite(grad).all()) and torch.equal(grad, grad0)
    assert bool(torch.isnan(buf[:4]).all()) and bool(torch.isnan(buf[4 + n:]).all()) and buf[4 + n:].numel() >= 4


def test_repeats_and_the_two_ends_of_lambda():
    import fused_loss
    C, H, W = 3, 33, 65
    x, y, *_ = _case(C, H, W)
    a_vals, a = fused_loss.l1_ssim_loss_and_grad(x, y, LAMBDA)
    b_vals, b = fused_loss.l1_ssim_loss_and_grad(x, y, LAMBDA)
    assert torch.equal(a_vals, b_vals) and torch.equal(a, b)
    # lambda = 0: L1 alone, whose gradient is sign(x - y) / (C H W) exactly
    vals, grad = fused_loss.l1_ssim_loss_and_grad(x, y, 0.0)
    inv_total = float(np.float32(1.0) / np.float32(C * H * W))
    assert torch.equal(grad, torch.sign(x - y) * inv_total)
    assert float(vals[0]) == float(vals[1])
    # lambda = 1: 1 - SSIM alone
    vals, grad = fused_loss.l1_ssim_loss_and_grad(x, y, 1.0)
    assert abs(float(vals[0]) - (1.0 - float(vals[2]))) <= 1e-7
    assert torch.equal(vals[1:], a_vals[1:])
