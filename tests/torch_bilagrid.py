"""The bilateral grid of affine colour transforms (include/gsr_bilagrid.h, fused_bilagrid.py) written out by hand in torch, without
grid_sample: the reference of tests/test_bilagrid_cpu.py and tests/test_bilagrid_gpu.py (float64 by default; dtype=torch.float32
gives the plain fp32 evaluation the gradient bars are scaled by).  Also the inputs those tests share.

    gx = (x + 0.5) / W * (GW - 1),  gy = (y + 0.5) / H * (GH - 1),  gz = clamp((0.299 r + 0.587 g + 0.114 b) (L - 1), 0, L - 1)
    A[c][k] = trilinear interpolation of channel 4c + k at (gz, gy, gx): cell floor() capped at size - 2, weights 1 - t, t
    out_c = A[c][0] r + A[c][1] g + A[c][2] b + A[c][3]
    tv = (1 / N) sum over the axes a of sum (g[i + 1 along a] - g[i])^2 / count_a
"""
import torch

LUMA = (0.299, 0.587, 0.114)


def spatial_cells(n_pixels, n_nodes, dtype=torch.float64):
    """-> (cell index (n_pixels,) long, weight t (n_pixels,)) of the pixel centres along one spatial axis"""
    g = (torch.arange(n_pixels, dtype=dtype) + 0.5) / n_pixels * (n_nodes - 1)
    c = g.floor().clamp(max=n_nodes - 2).long()
    return c, g - c.to(dtype)


def luma_coordinate(image, L):
    """-> luma * (L - 1), before the clamp, in the image's dtype"""
    return (LUMA[0] * image[0] + LUMA[1] * image[1] + LUMA[2] * image[2]) * (L - 1)


def luma_cells(image, L):
    """-> (cell index (H,W) long, gz (H,W) differentiable inside the range only, inside (H,W) bool)"""
    zf = luma_coordinate(image, L)
    inside = (zf > 0) & (zf < L - 1)
    gz = torch.where(inside, zf, zf.detach().clamp(0, L - 1))   # the border rule: no gradient through a clamped coordinate
    return gz.detach().floor().clamp(max=L - 2).long(), gz, inside


def transforms(grid, image):
    """-> A (12,H,W): the interpolated transform of every pixel (differentiable w.r.t. grid and, through gz, image)"""
    _, L, GH, GW = grid.shape
    _, H, W = image.shape
    cy, ty = spatial_cells(H, GH, grid.dtype)
    cx, tx = spatial_cells(W, GW, grid.dtype)
    cz, gz, _ = luma_cells(image, L)
    tz = gz - cz.to(grid.dtype)
    Y, X = cy[:, None].expand(H, W), cx[None, :].expand(H, W)
    TY, TX = ty[:, None], tx[None, :]
    A = 0
    for dz, wz in ((0, 1 - tz), (1, tz)):
        for dy, wy in ((0, 1 - TY), (1, TY)):
            for dx, wx in ((0, 1 - TX), (1, TX)):
                A = A + (wz * wy * wx) * grid[:, cz + dz, Y + dy, X + dx]
    return A


def slice(grid, image):   # noqa: A001  (gsplat's name)
    A = transforms(grid, image)
    return torch.stack([A[4 * c] * image[0] + A[4 * c + 1] * image[1] + A[4 * c + 2] * image[2] + A[4 * c + 3] for c in range(3)])


def slice_and_grads(grid, image, grad_out, dtype=torch.float64):
    """-> (out, {"grid", "image"} gradients for grad_out = dL/dout, affine part of dL/dimage, inside (H,W) bool), all in `dtype`"""
    g = grid.detach().to(dtype).requires_grad_(True)
    x = image.detach().to(dtype).requires_grad_(True)
    go = grad_out.detach().to(dtype)
    out = slice(g, x)
    dg, dx = torch.autograd.grad(out, (g, x), go)
    with torch.no_grad():
        A = transforms(g, x)
        affine = torch.stack([sum(A[4 * c + k] * go[c] for c in range(3)) for k in range(3)])
        inside = luma_cells(x, g.shape[1])[2]
    return out.detach(), {"grid": dg, "image": dx}, affine, inside


def total_variation(grids):
    """grids (N,12,L,GH,GW) or (12,L,GH,GW) -> scalar"""
    g = grids if grids.dim() == 5 else grids[None]
    N = g.shape[0]
    tv = 0
    for axis in (2, 3, 4):
        n = g.shape[axis]
        d = g.narrow(axis, 1, n - 1) - g.narrow(axis, 0, n - 1)
        tv = tv + (d * d).sum() / (d.numel() // N)
    return tv / N


def tv_and_grad(grids, dtype=torch.float64):
    g = grids.detach().to(dtype).requires_grad_(True)
    tv = total_variation(g)
    (dg,) = torch.autograd.grad(tv, g)
    return tv.detach(), dg


# ---- the inputs of the tests ----
MARGIN = 2e-3   # no pixel's luma coordinate lies this close to an integer: fp32 and fp64 then agree on every luma cell


def make_inputs(H, W, L, GH, GW, seed=5):
    """-> (grid (12,L,GH,GW), image (3,H,W), grad_out (3,H,W)) float32 CPU tensors built in float64: the grid is the identity plus
    0.2 N(0,1); the image is uniform in [-0.15, 1.15] with one block forced to 1.2 and one to -0.1 (both clamped sides of the luma
    axis occur), and every pixel whose luma (L - 1) lies within MARGIN of an integer gets 0.01 / (L - 1) added to its three channels."""
    g = torch.Generator().manual_seed(seed + 100000 * L + 1000 * GH + 100 * GW + 10 * H + W)
    eye = torch.eye(3, 4, dtype=torch.float64).reshape(12, 1, 1, 1)
    grid = (eye + 0.2 * torch.randn(12, L, GH, GW, generator=g, dtype=torch.float64)).float()
    x = -0.15 + 1.3 * torch.rand(3, H, W, generator=g, dtype=torch.float64)
    bh, bw = max(1, H // 4), max(1, W // 4)
    x[:, :bh, :bw] = 1.2
    x[:, H - bh:, W - bw:] = -0.1
    for _ in range(4):   # a nudged pixel may land next to the following integer only by 0.01 - 2 MARGIN > MARGIN: one round does it
        zf = luma_coordinate(x.float().double(), L)
        near = (zf - zf.round()).abs() <= MARGIN
        x = x + near.to(torch.float64) * (0.01 / (L - 1))
    grad_out = torch.randn(3, H, W, generator=g, dtype=torch.float64).float()
    return grid, x.float(), grad_out


def assert_inputs_are_safe(image, L, GH, GW):
    """On the CPU, before anything is compared: both clamped sides occur, no luma coordinate is within MARGIN of an integer, and
    the float32 and the float64 evaluation agree on every cell index."""
    _, H, W = image.shape
    zf = luma_coordinate(image.double(), L)
    assert bool((zf <= 0).any()) and bool((zf >= L - 1).any()) and bool(((zf > 0) & (zf < L - 1)).any())
    assert float((zf - zf.round()).abs().min()) > MARGIN
    assert torch.equal(luma_cells(image.float(), L)[0], luma_cells(image.double(), L)[0])
    assert torch.equal(luma_cells(image.float(), L)[2], luma_cells(image.double(), L)[2])
    for n_pixels, n_nodes in ((H, GH), (W, GW)):
        assert torch.equal(spatial_cells(n_pixels, n_nodes, torch.float32)[0], spatial_cells(n_pixels, n_nodes, torch.float64)[0])
