"""GPU: the backward blend's deferred finish (csrc/render_backward.hip).  The default kernel finishes its reduced instances four
at a time, and whatever is left at the end of each 64-instance batch.  One-tile scenes put a chosen count of reduced instances
into a batch: 1, 3 (one partial flush), 4 (one full flush), 5 (full + partial), 64 (sixteen full flushes) and 70 (a full batch,
then 4 + 2).  Then a heavy tile walked in depth segments, the culling switched off, and the depth-and-alpha (AUX) and
anti-aliased paths.  Each case is checked against the oracle with the bars of test_parity_gpu.py, and each is run twice: every
output must be the same bit for bit."""
import numpy as np
import pytest
import torch

import gsr_scene
import util
from test_parity_gpu import check_forward, check_grads

pytestmark = pytest.mark.gpu
GRADS = ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"]
DEV = torch.device("cuda:0")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _one_tile_scene(n, D=2, seed=0):
    """n Gaussians in front of a 16 x 16 image (one tile), all on it and faint enough that every one of them blends into
    pixels (T stays above 1e-4 behind all 70): each is a reduced instance of the tile's backward walk."""
    scene = gsr_scene.make_scene(n, float(np.log(0.08)), sh_degree=D, seed=seed)
    g = torch.Generator().manual_seed(100 + seed)
    means = (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([0.1, 0.1, 1.0])
    opac = 0.04 + 0.06 * torch.rand(n, 1, generator=g)
    scales = 0.06 + 0.06 * torch.rand(n, 3, generator=g)
    scene = scene._replace(means3D=means.contiguous(), opacities=opac.contiguous(), scales=scales.contiguous())
    return scene, gsr_scene.make_camera(16, 16, fovx=0.15)


def _heavy_scene():
    """A dense, low-opacity blob: a few tiles carry instance lists many times the mean and are walked in depth segments."""
    P, W, H, D = 40_000, 240, 160, 1
    scene = gsr_scene.make_scene(P, -3.6, sh_degree=D, seed=21)
    g = torch.Generator().manual_seed(22)
    nb = P * 3 // 4
    means = scene.means3D.clone()
    means[:nb] = torch.randn(nb, 3, generator=g) * torch.tensor([0.1, 0.07, 0.3])
    opac = scene.opacities.clone()
    opac[:nb] = torch.sigmoid(torch.randn(nb, 1, generator=g) - 3.5)
    return scene._replace(means3D=means.contiguous(), opacities=opac.contiguous()), gsr_scene.make_camera(W, H), D


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), f"{what}: two runs differ"


def _check_twice(scene, cam, D, seed, debug=False):
    """Oracle check of one run, then a second run bit for bit equal to the first (image, the blend sums, every gradient)."""
    o = util.oracle_forward(scene, cam, D)
    dpix = util.fragile_free_dpix(o, cam, seed=seed)
    h = util.hip_forward_backward(scene, cam, D, dpix, debug=debug)
    check_forward(h, o, cam)
    check_grads(h, o, dpix, GRADS)
    h2 = util.hip_forward_backward(scene, cam, D, dpix, debug=debug)
    _same_bits(h["color"], h2["color"], "color")
    for k in h["raw_grads"]:
        _same_bits(h["raw_grads"][k], h2["raw_grads"][k], k)
    for k in h["grads"]:
        _same_bits(h["grads"][k], h2["grads"][k], k)
    return o, h, dpix


@pytest.mark.parametrize("n", [1, 3, 4, 5, 64, 70])
def test_reduced_instances_per_batch(n):
    _need_gpu()
    scene, cam, D = *_one_tile_scene(n), 2
    o, h, _ = _check_twice(scene, cam, D, seed=n)
    # the case is what it claims: every Gaussian has an instance on the tile and blends into some pixel (a reduced instance)
    assert o["num_rendered"] == n
    assert np.all(h["raw_grads"]["dL_dopacity"] != 0), "a Gaussian without a hit: fewer reduced instances than intended"


def test_heavy_tile_depth_segments():
    _need_gpu()
    scene, cam, D = _heavy_scene()
    o, h, _ = _check_twice(scene, cam, D, seed=5)
    lens = h["ranges"][:, 1].astype(np.int64) - h["ranges"][:, 0]
    assert lens.max() >= 4 * 512, f"longest list {lens.max()}: no tile deep enough for depth segments"


@pytest.mark.parametrize("case", ["one_tile_70", "heavy"])
def test_cull_off(case):
    """GSR_DEBUG_NO_CULL stages every instance: other batch boundaries, other flush points, the same results."""
    _need_gpu()
    from diff_gaussian_rasterization import _C
    if case == "heavy":
        scene, cam, D = _heavy_scene()
    else:
        scene, cam, D = *_one_tile_scene(70), 2
    _, h_off, dpix = _check_twice(scene, cam, D, seed=6, debug=_C.DEBUG_NO_CULL)
    h_on = util.hip_forward_backward(scene, cam, D, dpix)
    for k in h_on["grads"]:
        _same_bits(h_on["grads"][k], h_off["grads"][k], f"{k} cull on / off")


def _leaves(scene):
    t = {k: getattr(scene, k).to(DEV).clone().requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    t["means2D"] = torch.zeros(scene.means3D.shape, device=DEV, requires_grad=True)
    return t


def _run(scene, cam, D, dpix, depth_alpha=None, dD=None, dA=None, antialiasing=False):
    from diff_gaussian_rasterization import GaussianRasterizer
    st = util.hip_settings(scene, cam, D, DEV)
    t = _leaves(scene)
    kw = {} if depth_alpha is None else {"depth_alpha": depth_alpha}
    out = GaussianRasterizer(st, antialiasing=antialiasing, **kw)(**t)
    loss = (out[0] * dpix.to(DEV)).sum()
    if dD is not None:
        loss = loss + (out[2] * dD.to(DEV)).sum()
    if dA is not None:
        loss = loss + (out[3] * dA.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return [x.detach().cpu().numpy() for x in out], {k: v.grad.cpu().numpy() for k, v in t.items()}


@pytest.mark.parametrize("case", ["one_tile_5", "heavy"])
def test_aux_path(case):
    """The AUX variant keeps the per-instance finish.  With zero dL/dD and dL/dA it runs its own kernel on the colour gradient
    alone, whose sums must equal the default path's (the deferred finish adds in the same trees); with random ones, two runs
    agree bit for bit."""
    _need_gpu()
    scene, cam, D = _heavy_scene() if case == "heavy" else (*_one_tile_scene(5), 2)
    H, W = cam.image_height, cam.image_width
    g = torch.Generator().manual_seed(8)
    dpix, dD, dA = torch.randn(3, H, W, generator=g), torch.randn(1, H, W, generator=g), torch.randn(1, H, W, generator=g)
    _, g_def = _run(scene, cam, D, dpix)
    _, g_aux0 = _run(scene, cam, D, dpix, "depth", torch.zeros(1, H, W), torch.zeros(1, H, W))
    for k in g_def:
        assert np.array_equal(g_def[k], g_aux0[k]), f"{k}: AUX with zero map gradients differs from the default path"
    o1, g1 = _run(scene, cam, D, dpix, "depth", dD, dA)
    o2, g2 = _run(scene, cam, D, dpix, "depth", dD, dA)
    for a, b in zip(o1, o2):
        _same_bits(a, b, "aux outputs")
    for k in g1:
        _same_bits(g1[k], g2[k], f"aux {k}")


@pytest.mark.parametrize("case", ["one_tile_64", "heavy"])
def test_antialiased_path(case):
    """antialiasing=True runs the default backward blend on the compensated opacities: two runs agree bit for bit.  (Its
    parity with the plain rasterizer fed the record opacity is test_antialias_gpu.py's.)"""
    _need_gpu()
    scene, cam, D = _heavy_scene() if case == "heavy" else (*_one_tile_scene(64), 2)
    dpix = torch.randn(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(9))
    o1, g1 = _run(scene, cam, D, dpix, antialiasing=True)
    o2, g2 = _run(scene, cam, D, dpix, antialiasing=True)
    for a, b in zip(o1, o2):
        _same_bits(a, b, "aa outputs")
    for k in g1:
        _same_bits(g1[k], g2[k], f"aa {k}")
        assert np.isfinite(g1[k]).all(), k
    assert np.abs(g1["opacities"]).max() > 0
