"""GPU: the backward blend's pair modes (csrc/render_backward.hip).  A lane's four pixels are two packed pairs, pair p holding
the 16x4-pixel bands 2p (.x halves) and 2p + 1 (.y halves) of the tile.  A pair whose two bands can both be reached runs the
packed body; a pair with one reachable band runs the same operations on that half alone; a band is unreachable for an instance
when the band mask says so or when the instance lies at or beyond the band's largest n_contrib.

One-tile scenes put a single small Gaussian on chosen bands -- every mode of either pair on its own, and `.y then .x` -- then
mix the modes inside batches and across a batch boundary; images cut by their edge leave whole bands without a pixel; opaque
Gaussians over the top half make the top bands finish early.  Then the 70-Gaussian tile through the depth-and-alpha, absgrad
and anti-aliased paths, a heavy tile walked in depth segments, and seeded random scenes.

Every case gets three checks: (i) the oracle / the path's reference composition with the existing bars of the suite it belongs
to, (ii) default against GSR_DEBUG_NO_CULL (every pair evaluated packed, like the reference): every gradient byte for byte,
(iii) two runs byte for byte."""
import math

import numpy as np
import pytest
import torch

import gsr_scene
import util
from test_parity_gpu import check_forward, check_grads

pytestmark = pytest.mark.gpu
GRADS = ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"]
DEV = torch.device("cuda:0")
FOVX = 0.15
UNIT = 4.0 * math.tan(FOVX / 2)   # half the image width in world units at the depth of the origin (camera at z = -4)
_cache = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), f"{what} differ"


def _rows_hit(o, W, H):
    """Per Gaussian: the image rows with alpha >= 1/255 at some pixel centre, in float64 from the oracle's mean, conic and
    opacity (forward.cu:330-350: power <= 0, alpha = min(0.99, o exp(power)))."""
    m, co = o["means2D"].astype(np.float64), o["conic_opacity"].astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    rows = []
    for i in range(m.shape[0]):
        dx, dy = m[i, 0] - xs, m[i, 1] - ys
        power = -0.5 * (co[i, 0] * dx * dx + co[i, 2] * dy * dy) - co[i, 1] * dx * dy
        alpha = np.minimum(0.99, co[i, 3] * np.exp(power))
        rows.append(np.nonzero(((power <= 0) & (alpha >= 1.0 / 255.0)).any(1))[0])
    return rows


def _pair_modes(o, W, H):
    """How many (Gaussian, tile row, pair) have mode 1 (.x band only), 2 (.y band only), 3 (both), by the footprints."""
    count = {1: 0, 2: 0, 3: 0}
    for rows in _rows_hit(o, W, H):
        for ty in range((H + 15) // 16):
            bands = {(r - 16 * ty) // 4 for r in rows if 16 * ty <= r < 16 * ty + 16}
            for p in (0, 1):
                m = (1 if 2 * p in bands else 0) | (2 if 2 * p + 1 in bands else 0)
                if m:
                    count[m] += 1
    return count


def _three_checks(scene, cam, D, seed, fragile_cap=0.02):
    from diff_gaussian_rasterization import _C
    o = util.oracle_forward(scene, cam, D)
    assert (o["fragile"] != 0).mean() <= fragile_cap, "too many fragile pixels: choose another seed"
    dpix = util.fragile_free_dpix(o, cam, seed=seed)
    h = util.hip_forward_backward(scene, cam, D, dpix)
    check_forward(h, o, cam)                                   # (i)
    check_grads(h, o, dpix, GRADS)
    h_off = util.hip_forward_backward(scene, cam, D, dpix, debug=_C.DEBUG_NO_CULL)
    _same_bits(h["color"], h_off["color"], "color, cull on / off")
    for k in h["grads"]:                                       # (ii)
        _same_bits(h["grads"][k], h_off["grads"][k], f"{k}, cull on / off")
    h2 = util.hip_forward_backward(scene, cam, D, dpix)
    _same_bits(h["color"], h2["color"], "color, two runs")
    for k in h["raw_grads"]:                                   # (iii)
        _same_bits(h["raw_grads"][k], h2["raw_grads"][k], f"{k}, two runs")
    for k in h["grads"]:
        _same_bits(h["grads"][k], h2["grads"][k], f"{k}, two runs")
    return o, h


def _world(px, py, W, H):
    """World x, y (at z = 0) of the pixel position (px, py): mean2D = ((ndc + 1) S - 1) / 2."""
    return ((2 * px + 1) / W - 1) * UNIT, ((2 * py + 1) / H - 1) * UNIT * H / W


# name: row of the centre, scale (world units, times (1, 0.5, 1.5) per axis; the screen-space dilation adds 0.3 px^2), opacity, the bands of the footprint
SINGLE = {
    "band0": (1.5, 0.004, 0.3, [0]), "band1": (5.5, 0.004, 0.3, [1]), "band2": (9.5, 0.004, 0.3, [2]), "band3": (13.5, 0.004, 0.3, [3]),
    "bands01": (3.5, 0.02, 0.3, [0, 1]), "bands23": (11.5, 0.02, 0.3, [2, 3]), "bands12": (7.5, 0.02, 0.3, [1, 2]),
    "bands0123": (7.5, 0.12, 0.5, [0, 1, 2, 3]),
}


@pytest.mark.parametrize("name", list(SINGLE))
def test_single_gaussian_on_chosen_bands(name):
    """One 16x16 tile, one Gaussian: each mode of each pair alone -- band k only (pair k / 2 in mode 1 or 2), bands 0-1 and 2-3
    (one packed pair), bands 1-2 (two one-band pairs, .y then .x), all four."""
    _need_gpu()
    row, scale, opacity, bands = SINGLE[name]
    cam = gsr_scene.make_camera(16, 16, fovx=FOVX)
    scene = gsr_scene.make_scene(1, 0.0, sh_degree=2, seed=1)
    x, y = _world(7.5, row, 16, 16)
    # (unequal axes: dL/drotations of a sphere is a sum of terms that cancel to nothing, and the oracle's own two fp32 summation
    # orders then differ by 1e-5 of it -- measured on the CPU for the band-2 case; with these axes they agree to 7e-7 in every case)
    scene = scene._replace(means3D=torch.tensor([[x, y, 0.0]]), opacities=torch.tensor([[opacity]]),
                           scales=scale * torch.tensor([[1.0, 0.5, 1.5]]))
    o, h = _three_checks(scene, cam, 2, seed=3)
    rows = _rows_hit(o, 16, 16)[0]
    assert sorted({int(r) // 4 for r in rows}) == bands, f"footprint rows {rows}: not the bands intended"
    assert o["num_rendered"] == 1
    assert h["raw_grads"]["dL_dopacity"][0] != 0, "the Gaussian was not blended"


def _tile_scene(n, seed, W=16, H=16, D=2):
    """The recipe of test_backward_flush_gpu._one_tile_scene with the scales reduced (0.1 ... 1.4 px before the dilation) and the
    centres spread over the image: faint Gaussians of small random footprints, one to four bands each."""
    scene = gsr_scene.make_scene(n, float(np.log(0.08)), sh_degree=D, seed=seed)
    g = torch.Generator().manual_seed(100 + seed)
    means = (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([1.8 * UNIT, 1.8 * UNIT * H / W, 1.0])
    opac = 0.04 + 0.06 * torch.rand(n, 1, generator=g)
    scales = 0.004 + 0.05 * torch.rand(n, 3, generator=g) ** 2
    scene = scene._replace(means3D=means.contiguous(), opacities=opac.contiguous(), scales=scales.contiguous())
    return scene, gsr_scene.make_camera(W, H, fovx=FOVX)


@pytest.mark.parametrize("n", [5, 64, 70])
def test_modes_mixed_in_a_batch(n):
    """5 (one partial flush), 64 (a full batch) and 70 (a batch boundary) Gaussians on one tile, all three modes among them."""
    _need_gpu()
    scene, cam = _tile_scene(n, 0)
    o, h = _three_checks(scene, cam, 2, seed=n)
    modes = _pair_modes(o, 16, 16)
    assert o["num_rendered"] == n and min(modes.values()) >= 1, f"modes {modes}: one of them is missing"


@pytest.mark.parametrize("W,H", [(16, 10), (20, 22)])
def test_tiles_cut_by_the_image_edge(W, H):
    """16x10: bands 2 (half) and 3 have no pixel.  20x22: the right tiles are 4 pixels wide, the lower ones hold bands 0 and
    half of 1."""
    _need_gpu()
    scene, cam = _tile_scene(40, 0, W, H)
    o, h = _three_checks(scene, cam, 2, seed=7)
    modes = _pair_modes(o, W, H)
    assert min(modes.values()) >= 1, f"modes {modes}: one of them is missing"


def _early_scene(seed=0, nfront=24, nback=40, D=2):
    """24 near-opaque wide Gaussians in front, centred on rows 1.5 and 5.5 (sigma_y 2.5 px): the top half of the tile is done after
    a dozen instances.  40 faint ones behind cover all of it."""
    n = nfront + nback
    scene = gsr_scene.make_scene(n, float(np.log(0.08)), sh_degree=D, seed=seed)
    g = torch.Generator().manual_seed(200 + seed)
    px = UNIT / 8   # one pixel in world units at z = 0
    means, opac, scales = torch.zeros(n, 3), torch.zeros(n, 1), torch.zeros(n, 3)
    means[:nfront, 0] = (torch.rand(nfront, generator=g) - 0.5) * 4 * px
    means[:nfront, 1] = (torch.where(torch.arange(nfront) % 2 == 0, 1.5, 5.5) - 7.5 + (torch.rand(nfront, generator=g) - 0.5)) * px
    means[:nfront, 2] = -1.0 + 0.5 * torch.rand(nfront, generator=g)
    opac[:nfront, 0] = 0.99
    scales[:nfront] = torch.tensor([12 * px, 2.5 * px, 0.01])
    means[nfront:] = (torch.rand(nback, 3, generator=g) - 0.5) * torch.tensor([0.1, 0.1, 1.0])
    means[nfront:, 2] += 0.6
    opac[nfront:, 0] = 0.04 + 0.06 * torch.rand(nback, generator=g)
    scales[nfront:] = 0.06 + 0.06 * torch.rand(nback, 3, generator=g)
    rot = torch.zeros(n, 4)
    rot[:, 0] = 1.0
    scene = scene._replace(means3D=means.contiguous(), opacities=opac.contiguous(), scales=scales.contiguous(), rotations=rot)
    return scene, gsr_scene.make_camera(16, 16, fovx=FOVX)


def test_bands_that_finish_early():
    """The top bands' largest n_contrib is smaller than the bottom bands': behind it, a pair of the walk has one band left."""
    _need_gpu()
    scene, cam = _early_scene()
    o, h = _three_checks(scene, cam, 2, seed=9)
    nc = h["n_contrib"].reshape(16, 16)
    last = [int(nc[4 * k:4 * k + 4].max()) for k in range(4)]
    assert max(last[0], last[1]) < min(last[2], last[3]), f"largest n_contrib per band {last}: the top bands do not finish early"
    assert last[0] < last[1], f"largest n_contrib per band {last}: pair 0 never has one band left"


def _tile70():
    if "tile70" not in _cache:
        _cache["tile70"] = _tile_scene(70, 0)
    return _cache["tile70"]


def _maps(seed, H, W):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(3, H, W, generator=g).to(DEV), torch.randn(1, H, W, generator=g).to(DEV), torch.randn(1, H, W, generator=g).to(DEV)


def test_tile70_depth_and_alpha():
    """The 70-Gaussian tile through GaussianRasterizer(depth_alpha="depth") against the two-pass composition, with
    test_depth_alpha_gpu.py's bars."""
    _need_gpu()
    from diff_gaussian_rasterization import _C
    import test_depth_alpha_gpu as da
    scene, cam = _tile70()
    dpix, dD, dA = _maps(11, 16, 16)
    f = da.fused(scene, cam, 2, "depth", dpix, dD, dA)
    r = da.two_pass(scene, cam, 2, "depth", dpix, dD, dA)
    da.check_forward(f, r)
    da.check_grads(f[4], r[3], da.two_pass(scene, cam, 2, "depth", dpix, dD, dA, split=True)[3], label="one-band tile70/depth")
    for label, debug in (("cull on / off", _C.DEBUG_NO_CULL), ("two runs", False)):
        f2 = da.fused(scene, cam, 2, "depth", dpix, dD, dA, debug=debug)
        for a, b in zip(f[:4], f2[:4]):
            _same_bits(a.cpu().numpy(), b.cpu().numpy(), f"outputs, {label}")
        for k in f[4]:
            _same_bits(f[4][k].cpu().numpy(), f2[4][k].cpu().numpy(), f"{k}, {label}")


@pytest.mark.parametrize("variant", ["absgrad", "absgrad_invdepth"])
def test_tile70_absgrad(variant):
    """... through absgrad, alone and together with the depth-and-alpha maps, against the float64 per-pixel terms with
    test_absgrad_gpu.py's bar; everything else the backward writes is what it is without absgrad."""
    _need_gpu()
    from diff_gaussian_rasterization import _C
    import test_absgrad_gpu as ab
    scene, cam = _tile70()
    o = util.oracle_forward(scene, cam, 2)
    dpix = util.fragile_free_dpix(o, cam, seed=3)
    kw, run_kw, dL = {}, {}, dpix
    if variant == "absgrad_invdepth":
        g = torch.Generator().manual_seed(5)
        dL = (dpix, torch.randn(16, 16, generator=g) * (dpix[0] != 0), torch.randn(16, 16, generator=g) * (dpix[0] != 0))
        kw["depth_mode"], run_kw["depth_alpha"] = "invdepth", "invdepth"
    ref, signed, d32 = ab._terms(scene, cam, dL, D=2, o=o, **kw)
    a = ab._run(scene, cam, dL, "both", D=2, **run_kw)
    ab._check(a["abs_mean2D"], ref, d32, f"one-band tile70 {variant}")
    ab._same_everything(a, ab._run(scene, cam, dL, None, D=2, **run_kw))
    for label, debug in (("cull on / off", _C.DEBUG_NO_CULL), ("two runs", False)):
        b = ab._run(scene, cam, dL, "both", D=2, debug=debug, **run_kw)
        ab._same_everything(a, b)
        _same_bits(a["abs_mean2D"].cpu().numpy(), b["abs_mean2D"].cpu().numpy(), f"abs_mean2D, {label}")
        _same_bits(a["accum"].cpu().numpy(), b["accum"].cpu().numpy(), f"accum, {label}")


def test_tile70_antialiased():
    """... with anti-aliasing, against the composition of test_antialias_gpu.py with its bars."""
    _need_gpu()
    from diff_gaussian_rasterization import _C
    import test_antialias_gpu as aa
    scene, cam = _tile70()
    aa._check(scene, cam, 2, "sh", "one-band tile70/aa")
    dpix, _, _ = aa._dpix(1, 16, 16)
    f, g = aa.fused(scene, cam, 2, "sh", dpix)
    for label, debug in (("cull on / off", _C.DEBUG_NO_CULL), ("two runs", 0)):
        f2, g2 = aa.fused(scene, cam, 2, "sh", dpix, debug=debug)
        for a, b in zip(f, f2):
            _same_bits(a.cpu().numpy(), b.cpu().numpy(), f"outputs, {label}")
        for k in g:
            _same_bits(g[k].cpu().numpy(), g2[k].cpu().numpy(), f"{k}, {label}")


def test_heavy_tile_depth_segments():
    """test_backward_flush_gpu._heavy_scene: depth segments start in the middle of a list, each with its own largest n_contrib
    per band still ahead of it."""
    _need_gpu()
    from test_backward_flush_gpu import _heavy_scene
    scene, cam, D = _heavy_scene()
    o, h = _three_checks(scene, cam, D, seed=5)
    lens = h["ranges"][:, 1].astype(np.int64) - h["ranges"][:, 0]
    assert lens.max() >= 4 * 512, f"longest list {lens.max()}: no tile deep enough for depth segments"


@pytest.mark.parametrize("seed", range(6))
def test_random_scenes(seed):
    """The ranges of test_boundary_gpu.test_band_culling_changes_nothing's fuzz case: cameras inside the cloud, odd sizes, big
    splats."""
    _need_gpu()
    rng = np.random.default_rng(100 + seed)
    P = int(rng.integers(500, 6000))
    W, H = int(rng.integers(40, 400)), int(rng.integers(30, 260))
    D = int(rng.integers(0, 4))
    mu = float(rng.uniform(-3.5, -1.0))
    scene = gsr_scene.make_scene(P, mu, sh_degree=D, seed=seed)
    cam = gsr_scene.ring_camera(W, H, int(rng.integers(0, 8)), 8, radius=float(rng.uniform(0.3, 4.5)))
    _three_checks(scene, cam, D, seed=seed)
