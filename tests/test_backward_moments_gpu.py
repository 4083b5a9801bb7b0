"""GPU: the backward blend's geometric words from three lane sums (csrc/render_backward.hip).  Per evaluated pixel pair the kernel
accumulates sum g, sum g dy and sum g dy^2, g = G dL/dalpha; a lane's dx (its four pixels share their column) meets the lane's sums
once per reduced instance (sum g dx = dx sum g, sum g dx^2 = dx (dx sum g), sum g dx dy = dx sum g dy), and so does the instance's
opacity, which every staged instance reads from its own record: the five geometric values a lane hands to the wave reduction are
sums of f = o g as before.  dL/dopacity and dL/dcolor are formed as before.

Every case: the blend sums (raw_grads, as tests/test_grad_rows_gpu.py takes them) row by row and component by component within
oracle.blend_backward_budget's float64 bound E = 2^-24 (B + n A) through grad_rows.rows_failures -- the bound budgets four products
for a conic word and five products and a sum for a dL/dmean2D word along any path, which is what the kernel still spends, some of
the roundings now on a lane's sum instead of on a pixel's term -- and a second run with the same bits.  The scenes are tests/moment_scenes.py's; that the bound
is not vacuous on them (grad_rows.cap_shares) and that they are what they are named after is checked from the oracle alone by
tests/test_backward_moments_cpu.py.  The heavy tile's depth segments are test_grad_rows_gpu.test_deep_and_wide's."""
import numpy as np
import pytest
import torch

import grad_rows as gr
import moment_scenes as ms
import util

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), f"{what}: the bits differ"


def _rows_twice(scene, cam, label, ramp=0.0):
    """Every row of the four blend tensors within its float64 bound; a second run with the same bits.  -> (oracle state, run)"""
    o = util.oracle_forward(scene, cam, 0)
    dpix = gr.smooth_dpix(o, cam, ramp=ramp)
    bud = util.oracle.blend_backward_budget(o, dpix.numpy())
    h = util.hip_forward_backward(scene, cam, 0, dpix)
    ratios, bad = gr.rows_failures(h["raw_grads"], bud)
    msg = gr.format_ratios(ratios)
    print(f"[{label}]\n{msg}")
    util.parity_log(f"[moments/{label}] blend sums per row: largest |hip - float64| / E\n" + msg)
    assert not bad, f"[{label}] a row of the blend sums lies outside its float64 bound:\n" + "\n".join(bad) + "\n" + msg
    h2 = util.hip_forward_backward(scene, cam, 0, dpix)
    _same_bits(h["color"], h2["color"], "color")
    for k in h["raw_grads"]:
        _same_bits(h["raw_grads"][k], h2["raw_grads"][k], k)
    for k in h["grads"]:
        _same_bits(h["grads"][k], h2["grads"][k], k)
    return o, h


@pytest.mark.parametrize("name", ["centre", "left", "needle"])
def test_one_gaussian(name):
    """16 x 16, one Gaussian: inside the tile; 50 px to its left (one sign of dx in every lane, |dx| >> |dy|); a diagonal needle."""
    _need_gpu()
    scene, cam, ramp = ms.single(name)
    o, h = _rows_twice(scene, cam, name, ramp)
    assert o["num_rendered"] == 1 and h["raw_grads"]["dL_dopacity"][0] != 0, "the Gaussian was not blended"


def test_partial_tiles():
    """17 x 33: lanes outside the image in the one-pixel column, a tile row with one row of pixels (three bands wholly outside)."""
    _need_gpu()
    scene, cam = ms.odd_image()
    o, h = _rows_twice(scene, cam, "17 x 33")
    lens = h["ranges"][:, 1].astype(np.int64) - h["ranges"][:, 0]
    assert lens.shape[0] == 6 and (lens > 0).all(), f"list lengths {lens}: a tile without an instance"


def test_one_band_of_a_pair():
    """Footprints of one band each: pair 0 in mode 1 and in mode 2, pair 1 in mode 1 and in mode 2 -- the plain fp32 bodies,
    whose accumulators are one half of a register pair next to a -0."""
    _need_gpu()
    scene, cam = ms.one_band()
    o, h = _rows_twice(scene, cam, "one band")
    assert (h["raw_grads"]["dL_dopacity"].reshape(-1) != 0).all()


@pytest.mark.parametrize("n", ms.ONE_TILE_COUNTS)
def test_opacity_per_pending_instance(n):
    """One tile, n reduced instances of pairwise distinct opacities: partial, full and several flushes, a whole batch, a batch
    boundary.  The opacity now meets sums, not terms: a row scaled by another instance's opacity is off by at least the spacing
    of the opacities, 0.8 / (n - 1) of 0.9 at best: more than 1 %, against a bound below 1e-3 of the row (cap_shares)."""
    _need_gpu()
    scene, cam = ms.one_tile(n)
    o, h = _rows_twice(scene, cam, f"one tile, {n}")
    assert o["num_rendered"] == n and (h["raw_grads"]["dL_dopacity"].reshape(-1) != 0).all(), "an instance was not reduced"


NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")


def _through(scene, cam, dpix, absgrad, depth_alpha):
    """One forward and one backward of the image loss through the extension's functions, so that the blend kernel is the one of
    (depth-and-alpha, absgrad) whatever the loss holds: no dL/dD, no dL/dA.  -> (image, the eight gradients, abs_mean2D)"""
    from diff_gaussian_rasterization import _C
    dev = torch.device("cuda:0")
    W, H = cam.image_width, cam.image_height
    st = util.hip_settings(scene, cam, 0, dev)
    e = torch.empty(0, device=dev)
    t = {k: getattr(scene, k).to(dev) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    P = t["means3D"].shape[0]
    fwd = (st.bg, t["means3D"], e, t["opacities"], t["scales"], t["rotations"], 1.0, e, st.viewmatrix, st.projmatrix, st.tanfovx,
           st.tanfovy, H, W, t["shs"], 0, st.campos, False, False)
    am = torch.full((P, 2), float("nan"), device=dev) if absgrad else None
    kw = dict(absgrad=(am, torch.zeros(P, device=dev))) if absgrad else {}
    if depth_alpha:
        R, color, radii, geom, binning, img, _, _, aux = _C.rasterize_gaussians_depth_alpha(depth_alpha, *fwd)
    else:
        R, color, radii, geom, binning, img = _C.rasterize_gaussians(*fwd)
    bwd = (st.bg, t["means3D"], radii, e, t["scales"], t["rotations"], 1.0, e, st.viewmatrix, st.projmatrix, st.tanfovx, st.tanfovy,
           dpix.to(dev), t["shs"], 0, st.campos, geom, R, binning, img)
    if depth_alpha:
        g = _C.rasterize_gaussians_backward_depth_alpha(depth_alpha, *bwd, aux, None, None, False, **kw)
    else:
        g = _C.rasterize_gaussians_backward(*bwd, False, lean=True, **kw)
    torch.cuda.synchronize()
    return color.cpu().numpy(), {k: v.cpu().numpy() for k, v in zip(NAMES, g) if v is not None}, am


@pytest.mark.parametrize("n", [4, 5, 64, 65])
def test_aux_and_abs_kernels(n):
    """The one-tile scenes through the three other instantiations (depth-and-alpha, absgrad, both), which finish every instance
    on its own: without dL/dD and dL/dA their nine words are the default kernel's, so every gradient the backward returns equals
    the default's bit for bit; the sums of moduli stay within test_absgrad_gpu.py's bar against the float64 per-pixel terms."""
    _need_gpu()
    import test_absgrad_gpu as ab
    scene, cam = ms.one_tile(n)
    o = util.oracle_forward(scene, cam, 0)
    dpix = gr.smooth_dpix(o, cam)
    image, base, _ = _through(scene, cam, dpix, False, None)
    assert np.abs(base["dL_dmeans2D"]).max() > 0 and base["dL_dscales"].size == 3 * n
    ref, signed, d32 = ab._terms(scene, cam, dpix, D=0, o=o)
    for absgrad, depth_alpha in ((False, "depth"), (True, None), (True, "depth")):
        label = f"one tile, {n}: absgrad {absgrad}, depth_alpha {depth_alpha}"
        im, g, am = _through(scene, cam, dpix, absgrad, depth_alpha)
        _same_bits(im, image, f"image ({label})")
        assert g.keys() == base.keys(), label
        for k in base:
            _same_bits(g[k], base[k], f"{k} ({label})")
        if absgrad:
            ab._check(am, ref, d32, label)
