"""GPU: the trim words (csrc/gsr_rect_trim.h) and the band culling (render_common.h gsr_tile_band_mask) under long needles whose
centre lies far off the pixels they cover.

tests/test_trim_gpu.py decides "can contribute" in float64 on random scenes with needles of at most 30 : 1.  The blend kernels
decide it in fp32, in the reference's operation order (gsr_pair_power), and for a needle 1000 px long, 0.55 px thick, centred
thousands of pixels outside the image, both the conic's fp32 determinant and that fp32 `power` are far from the exact values:
a bound with constant margins trims tiles whose pixels the kernels blend ("The trim bound in fp32").  Here:

  * the family of tests/trim_reference.py (needle_cases: L 400 .. 1500 px, six angles, three opacities, the long axis through a point
    of the image, the centre 1, 2, 2.8 L along it), built as 3D Gaussians in a plane of constant view depth and rendered twelve at
    a time (the six angles through two points: they cross, they do not saturate T);
  * every decision from what the device wrote: means2D, conic, opacity, rectangle, trim word;
  * check A: every tile with a pixel that passes the kernels' accept test in the kernels' arithmetic (trim_reference.must_keep:
    power <= 0 and opacity exp(power) >= (1 + 1e-5) / 255) is kept, and the list holds exactly the kept instances;
  * check B: default against GSR_DEBUG_NO_TRIM -- image, final T, radii, tiles_touched, slot_base, every gradient bit for bit,
    n_contrib through the kept-prefix count;
  * check C: default against GSR_DEBUG_NO_CULL -- image, final T, n_contrib, every gradient bit for bit;
  * A and B once more with antialiasing, where the trim sees the compensated opacity.
"""
import math

import numpy as np
import pytest
import torch

import gsr_scene
import trim_reference as tr
import util

pytestmark = pytest.mark.gpu

SIZES = [(256, 256), (640, 368)]
PARTS = 4


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _groups(opacities=tr.NEEDLE_OPACITY):
    """The family in renders of twelve: one (L, opacity, k), the six angles through the two anchors."""
    return [[(L, th, o, k, an) for th in tr.NEEDLE_THETA for an in tr.NEEDLE_ANCHOR]
            for L in tr.NEEDLE_L for o in opacities for k in tr.NEEDLE_K]


def _scene(cases, cam, thin=1e-4):
    means, scales, rots, ops = tr.needle_3d(cases, cam)
    scales[:, 1:] = thin
    n = len(cases)
    g = torch.Generator().manual_seed(len(cases) + int(cases[0][0]))
    shs = torch.randn(n, 1, 3, generator=g)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    return gsr_scene.Scene(t(means), t(scales), t(rots), t(ops), shs.contiguous(), torch.zeros(3))


def _judge(h, cases, W, H):
    """Check A's evidence for one render, from the device's own fp32 values: per needle (case, visible, must (h, w), kept (h, w),
    score (h, w), tile ids (h, w), magnitude of the cancelling terms, ca cc / det in float64)."""
    gx = (W + 15) // 16
    rs, m2, co = h["rshape"], h["means2D"], h["conic_opacity"]
    out = []
    for g, case in enumerate(cases):
        if h["tiles_touched"][g] == 0:
            out.append((case, False, None, None, None, None, 0.0, 0.0))
            continue
        packed = int(rs[g, 0])
        rect = (packed & 255, (packed >> 8) & 255, ((packed >> 16) & 255) + 1, (packed >> 24) + 1)
        assert rect[2] * rect[3] == int(h["tiles_touched"][g])
        must, score, mag = tr.must_keep(m2[g, 0], m2[g, 1], co[g, 0], co[g, 1], co[g, 2], co[g, 3], rect, W, H)
        ty, tx = np.meshgrid(np.arange(rect[1], rect[1] + rect[3]), np.arange(rect[0], rect[0] + rect[2]), indexing="ij")
        tiles = ty * gx + tx
        kept = util.trim_kept(rs, np.full(tiles.size, g), tiles.reshape(-1), gx).reshape(tiles.shape)
        a, b, c = (float(co[g, j]) for j in range(3))
        det = a * c - b * b
        out.append((case, True, must, kept, score, tiles, mag, a * c / det if det > 0 else math.inf))
    return out


def _assert_adversarial_then_sound(judged, renders, W, H, tag):
    """The three shares that make the inputs adversarial first, then check A."""
    flat = [j for js in judged for j in js]
    n = len(flat)
    big = sum(j[6] >= 1e5 for j in flat)
    ill = sum(j[7] >= 1e4 for j in flat)
    need = sum(bool(j[1] and j[2].any()) for j in flat)
    tiles = sum(j[2].size for j in flat if j[1])
    kept_n = sum(int(j[3].sum()) for j in flat if j[1])
    must_n = sum(int(j[2].sum()) for j in flat if j[1])
    closest = max([float(j[4][~j[3]].max()) for j in flat if j[1] and (~j[3]).any()], default=-math.inf)
    line = (f"[trim needles {tag}] {n} needles: {big} with cancelling terms >= 1e5, {ill} with ca cc / det >= 1e4, {need} with a tile that must be kept; "
            f"{tiles} tiles, {must_n} must be kept, {kept_n} kept ({kept_n / max(tiles, 1):.3f}); closest trimmed pixel: power + ln(255 o) = {closest:+.3f}")
    print(line)
    util.parity_log(line)
    assert 3 * big >= n and 3 * ill >= n and need >= 0.8 * n, line
    lost = []
    for case, vis, must, kept, score, tiles_, _, _ in flat:
        if not vis:
            continue
        bad = must & ~kept
        if bad.any():
            i = np.unravel_index(np.argmax(np.where(bad, score, -np.inf)), bad.shape)
            lost.append((float(score[i]), case, int(bad.sum()), int(tiles_[i])))
    if lost:
        lost.sort(reverse=True)
        s, case, nb, tile = lost[0]
        L, th, o, k, an = case
        _, px, py = tr.needle_2d(case, W, H)
        raise AssertionError(f"{tag}: {len(lost)} needles lose a tile that holds a pixel the blend kernels accept.  Worst: L {L} px, theta {th} deg, opacity {o}, "
                             f"centre ({px:.1f}, {py:.1f}) (k = {k}), {nb} tiles, tile {tile}, power + ln(255 o) = {s:+.3f}; all: "
                             + "; ".join(f"L {c[0]} theta {c[1]} o {c[2]} k {c[3]} anchor {c[4]}: {v:+.3f}" for v, c, _, _ in lost[:40]))
    for js, h in zip(judged, renders):
        kept_total = sum(int(j[3].sum()) for j in js if j[1])
        listed = len(h["point_list"]) if h["num_rendered"] > 0 else 0
        assert listed == kept_total, f"{tag}: the list holds {listed} instances, the trim words keep {kept_total}"
    assert kept_n < tiles, "nothing was trimmed at all"


def _assert_no_output_can_tell(d, a, W, H, tag):
    """Check B: d the default lists, a the whole lists (GSR_DEBUG_NO_TRIM), both without depth segments."""
    gx = (W + 15) // 16
    for k in ("color", "final_T", "radii", "tiles_touched", "slot_base"):
        assert np.array_equal(d[k], a[k]), (tag, k)
    assert d["num_rendered"] == a["num_rendered"] == int(a["tiles_touched"].astype(np.int64).sum())
    for k in a["grads"]:
        assert np.array_equal(d["grads"][k], a["grads"][k]), (tag, k)
    assert a["num_rendered"] > 0 and not a["rshape"][:, 1].any() and len(a["point_list"]) == a["num_rendered"]
    T = gx * ((H + 15) // 16)
    r0 = a["ranges"].astype(np.int64)
    tile_of = np.repeat(np.arange(T, dtype=np.int64), r0[:, 1] - r0[:, 0])
    kept = util.trim_kept(d["rshape"], a["point_list"], tile_of, gx)
    assert np.array_equal(d["point_list"], a["point_list"][kept]), tag
    kcum = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    ys, xs = np.divmod(np.arange(W * H, dtype=np.int64), W)
    tp = (ys // 16) * gx + xs // 16
    n = a["n_contrib"].astype(np.int64)
    assert np.array_equal(d["n_contrib"].astype(np.int64), kcum[r0[tp, 0] + n] - kcum[r0[tp, 0]]), (tag, "n_contrib")


def _run_family(groups, W, H, tag, antialiasing=False, thin=1e-4, band_culling=True):
    from diff_gaussian_rasterization import _C
    cam = gsr_scene.make_camera(W, H)
    dpix = torch.randn(3, H, W, generator=torch.Generator().manual_seed(3))
    ns = _C.DEBUG_NO_SPLIT   # (no depth segments: their cuts fall on list positions, which differ between the two lists)
    kw = dict(antialiasing=antialiasing)
    scenes = [_scene(cases, cam, thin) for cases in groups]
    defaults = [util.hip_forward_backward(s, cam, 0, dpix, debug=ns, **kw) for s in scenes]
    judged = [_judge(h, cases, W, H) for h, cases in zip(defaults, groups)]
    _assert_adversarial_then_sound(judged, defaults, W, H, tag)
    for i, (s, d) in enumerate(zip(scenes, defaults)):
        a = util.hip_forward_backward(s, cam, 0, dpix, debug=ns | _C.DEBUG_NO_TRIM, **kw)
        _assert_no_output_can_tell(d, a, W, H, f"{tag} render {i} (L {groups[i][0][0]}, opacity {groups[i][0][2]}, k {groups[i][0][3]})")
        if not band_culling:
            continue
        p = util.hip_forward_backward(s, cam, 0, dpix, **kw)
        c = util.hip_forward_backward(s, cam, 0, dpix, debug=_C.DEBUG_NO_CULL, **kw)
        for k in ("color", "final_T", "n_contrib"):
            assert np.array_equal(p[k], c[k]), (tag, i, "band culling", k)
        for k in c["grads"]:
            assert np.array_equal(p["grads"][k], c["grads"][k]), (tag, i, "band culling", k)


@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("W,H", SIZES)
def test_needles_trim_is_sound_and_no_output_can_tell(W, H, part):
    _need_gpu()
    _run_family(_groups()[part::PARTS], W, H, f"{W}x{H} part {part}")


@pytest.mark.parametrize("half", range(2))
def test_needles_antialiased(half):
    """Checks A and B with antialiasing for the opacity-0.3 needles at 640x368: the trim then sees opacity * rho.  The thin axis is one
    pixel here, not a line: the filter's compensation of a line is the clamp 0.005, and opacity 0.0015 reaches no pixel at all."""
    _need_gpu()
    W, H = 640, 368
    cam = gsr_scene.make_camera(W, H)
    thin = 1.0 * 4.0 / (W / (2.0 * cam.tanfovx))
    _run_family(_groups(opacities=(0.3,))[half::2], W, H, f"{W}x{H} antialiased half {half}", antialiasing=True, thin=thin, band_culling=False)
