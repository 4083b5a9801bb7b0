"""CPU: the algebra of the trim bound (csrc/gsr_rect_trim.h gsr_rect_trim()) against the blend kernels' own accept test, on needles.

tests/trim_reference.py restates gsr_rect_trim() in scalar np.float32, operation for operation (reciprocal, square root and
logarithm correctly rounded where the device's are 1 ulp).  A CHANGE OF gsr_rect_trim() HAS TO BE REPEATED THERE: this test then
says, on a machine without a GPU, whether the changed bound still keeps every tile that can contribute.  What the device's own
words do is decided by tests/test_trim_needles_gpu.py.

"Can contribute" is decided as the kernels decide it (trim_reference.must_keep): fp32, the operation order of gsr_pair_power,
d = mean - pixel; a tile must be kept if a pixel centre of it inside the image has power <= 0 and
opacity exp(power) >= (1 + 1e-5) / 255.

The needle family: cov2D = R(theta) diag(L^2, 0.3) R(theta)^T in fp32, conic / radius / rectangle as the reference forms them,
L 400 .. 1500 px, six angles, three opacities, the long axis through a point of the image and the centre 1, 2 or 2.8 L along it --
thousands of pixels outside the image.  There the conic's fp32 determinant is off by percents and the kernels' fp32 `power` by up to 1
from the exact quadratic; a bound with constant margins loses tiles whose pixels reach five times the threshold ("The
trim bound in fp32").
"""
import numpy as np
import pytest

import trim_reference as tr

SIZES = [(256, 256), (640, 368)]


def _run(cov, px, py, opacity, W, H):
    """-> None if the reference drops the splat, else (must (h, w), kept (h, w), score (h, w), magnitude, ca cc / det in float64)."""
    g = tr.conic_radius_rect(cov, px, py, W, H)
    if g is None:
        return None
    (ca, cb, cc), _, rect = g
    trim = tr.rect_trim(tr.F(px), tr.F(py), ca, cb, cc, tr.F(opacity), *rect)
    must, score, mag = tr.must_keep(tr.F(px), tr.F(py), ca, cb, cc, tr.F(opacity), rect, W, H)
    kept = tr.kept_tiles(trim, rect, (W + 15) // 16)
    a, b, c = float(ca), float(cb), float(cc)
    return must, kept, score, mag, a * c / (a * c - b * b)


@pytest.mark.parametrize("W,H", SIZES)
def test_needles_no_tile_that_the_kernels_would_blend_is_trimmed(W, H):
    cases = tr.needle_cases()
    assert len(cases) == 864
    n = with_must = big_mag = ill = 0
    tiles = kept_n = must_n = 0
    lost, closest = [], -np.inf
    for case in cases:
        cov, px, py = tr.needle_2d(case, W, H)
        r = _run(tuple(tr.F(v) for v in cov), px, py, case[2], W, H)
        if r is None:
            continue
        must, kept, score, mag, cond = r
        n += 1
        with_must += bool(must.any()); big_mag += mag >= 1e5; ill += cond >= 1e4
        tiles += must.size; kept_n += int(kept.sum()); must_n += int(must.sum())
        bad = must & ~kept
        if bad.any():
            lost.append((case, int(bad.sum()), float(score[bad].max())))
        if (~kept).any():
            closest = max(closest, float(score[~kept].max()))
    print(f"[trim needles, {W}x{H}] {n} needles, {with_must} with a tile that must be kept, {big_mag} with cancelling terms >= 1e5, "
          f"{ill} with ca cc / det >= 1e4; {tiles} tiles, {must_n} must be kept, {kept_n} kept ({kept_n / tiles:.3f}); "
          f"closest trimmed pixel: power + ln(255 o) = {closest:+.3f}")
    # the family is what it is meant to be
    assert n == 864
    assert 3 * big_mag >= n and 3 * ill >= n and with_must >= 0.8 * n
    worst = max(lost, key=lambda v: v[2]) if lost else None
    assert not lost, (f"{len(lost)} needles lose a tile a pixel of which passes the kernels' accept test; the worst: (L, theta, opacity, k, anchor) = "
                      f"{worst[0]}, {worst[1]} tiles, power + ln(255 o) = {worst[2]:+.3f}")
    assert kept_n < tiles   # (and it still trims)


def test_ordinary_splats_none_lost_and_still_trimmed():
    W, H = 640, 368
    tiles = kept_n = 0
    closest = -np.inf
    for cov, px, py, o in tr.ordinary_cases(600, W, H, seed=1):
        r = _run(tuple(tr.F(v) for v in cov), px, py, o, W, H)
        if r is None:
            continue
        must, kept, score, _, _ = r
        bad = must & ~kept
        assert not bad.any(), f"cov2D {cov}, centre ({px}, {py}), opacity {o}: {int(bad.sum())} tiles lost, power + ln(255 o) = {float(score[bad].max()):+.3f}"
        tiles += must.size; kept_n += int(kept.sum())
        if (~kept).any():
            closest = max(closest, float(score[~kept].max()))
    share = 1.0 - kept_n / tiles
    print(f"[trim ordinary] {tiles} tiles of 600 splats, trimmed share {share:.3f}, closest trimmed pixel {closest:+.3f}")
    assert share > 0.0


def test_restated_decoder_shifts_match_the_header():
    """col_shift / row_shift here against their definition: the smallest power of two with at most 8 groups / 16 units."""
    for w in range(1, 257):
        s = tr.col_shift(w)
        assert (w + (1 << s) - 1) >> s <= 8 and (s == 0 or (w + (1 << (s - 1)) - 1) >> (s - 1) > 8)
    for h in range(1, 257):
        s = tr.row_shift(h)
        assert (h + (1 << s) - 1) >> s <= 16 and (s == 0 or (h + (1 << (s - 1)) - 1) >> (s - 1) > 16)
