"""Scenes of tests/test_backward_moments_gpu.py (the backward blend's geometric words formed from sum g, sum g dy, sum g dy^2 with
g = G dL/dalpha: dx and the opacity applied to a lane's sums, csrc/render_backward.hip), with what each has to be, checked
from the CPU oracle alone by tests/test_backward_moments_cpu.py.  All are degree-0 scenes under grad_rows.smooth_dpix; each keeps
grad_rows.cap_shares >= CAP_SHARE at CAP, so the per-row bound they are held to is not vacuous."""
import math

import numpy as np
import torch

import grad_rows as gr
import gsr_scene

FOVX = 0.15
ONE_TILE_COUNTS = (1, 3, 4, 5, 64, 65)


def _one(px, py, radius, opacity, W=16, H=16, seed=80):
    return gr._scene(np.array([px]), np.array([py]), np.array([4.0]), np.array([float(radius)]), np.array([opacity]), W, H, FOVX, seed)


def single(name):
    """One 16 x 16 image, one Gaussian.
    centre  the mean inside the tile: dx takes both signs over the lanes.
    left    the mean about 50 pixels left of the tile's centre (sigma 24 px): dx has one sign in every lane and is large against
            dy, so sum g dx and sum g dx^2 are where a lane's dx meets a sum it was not applied to pixel by pixel.
    needle  sigma 6.1 x 0.94 px along the diagonal through the tile (conic 0.584, 0.557, 0.584): dx and dy are equal and opposite
            along it, and the two products of dL/dmean2D cancel.  The thinnest that keeps the cap on dL/dmean2D: the row's
            A = sum |a f dx| + |b f dy| grows with the aspect ratio squared against its sum (thinner by a quarter: E = 2e-3 |S|), and
            only under an upstream gradient with a slope across the needle (smooth_dpix's ramp, e-folding length 4 px; without it
            the row cancels by symmetry to 7e-3).
    -> (scene, camera, ramp of grad_rows.smooth_dpix)"""
    cam = gsr_scene.make_camera(16, 16, fovx=FOVX)
    if name == "centre":
        return _one(6.3, 8.6, 12, 0.6), cam, 0.0
    if name == "left":
        return _one(-42.0, 7.0, 72, 0.9), cam, 0.0
    assert name == "needle"
    scene = _one(7.7, 7.2, 12, 0.8)
    s = float(scene.scales[0, 0])   # 12 px radius: sigma 3.8 px
    a = -math.pi / 8   # half of 45 degrees about the viewing axis: the needle lies across the ramp's direction (1, 1)
    return scene._replace(scales=torch.tensor([[s * 1.6, s * 0.2, s]]), rotations=torch.tensor([[math.cos(a), 0.0, 0.0, math.sin(a)]])), cam, 4.0


def odd_image(P=40):
    """17 x 33: two columns and three rows of tiles.  The right column is one pixel wide (15 of a wave's 16 columns outside the
    image), the bottom row one pixel high (bands 1-3 wholly outside, band 0 with one row)."""
    W, H = 17, 33
    rng = np.random.RandomState(5)
    px, py = rng.rand(P) * (W + 4) - 2, rng.rand(P) * (H + 4) - 2
    px[:4], py[:4] = [16.2, 15.8, 8.0, 16.4], [5.0, 20.0, 32.3, 32.6]   # on the narrow column, the low row and the corner
    scene = gr._scene(px, py, 3.5 + rng.rand(P), rng.randint(3, 9, size=P).astype(np.float64), 0.15 + 0.5 * rng.rand(P), W, H, FOVX, seed=81)
    return scene, gsr_scene.make_camera(W, H, fovx=FOVX)


BAND_ROWS = (1.5, 5.5, 9.5, 13.5)


def one_band():
    """One tile, eight Gaussians of sigma 0.57 px (little more than the 0.3 px^2 dilation) centred on rows 1.5, 5.5, 9.5, 13.5: each reaches one band, so pair 0
    runs in mode 1 (band 0) and in mode 2 (band 1), pair 1 in mode 1 (band 2) and in mode 2 (band 3), and never packed."""
    px = np.array([3.3, 11.6, 5.4, 12.7, 2.6, 9.3, 6.2, 13.4])
    py = np.array([BAND_ROWS[i // 2] for i in range(8)]) + np.array([0.1, -0.2, 0.2, -0.1, -0.15, 0.05, 0.1, -0.1])
    scene = gr._scene(px, py, np.linspace(3.6, 4.4, 8), np.full(8, 2.2), np.linspace(0.3, 0.8, 8), 16, 16, FOVX, seed=82)
    return scene, gsr_scene.make_camera(16, 16, fovx=FOVX)


def rows_hit(o, W, H):
    """Per Gaussian: the image rows with alpha >= 1/255 at some pixel centre, in float64 from the oracle's mean, conic and opacity."""
    m, co = o["means2D"].astype(np.float64), o["conic_opacity"].astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    rows = []
    for i in range(m.shape[0]):
        dx, dy = m[i, 0] - xs, m[i, 1] - ys
        power = -0.5 * (co[i, 0] * dx * dx + co[i, 2] * dy * dy) - co[i, 1] * dx * dy
        alpha = np.minimum(0.99, co[i, 3] * np.exp(power))
        rows.append(np.nonzero(((power <= 0) & (alpha >= 1.0 / 255.0)).any(1))[0])
    return rows


def one_tile(n):
    """One tile, n Gaussians of pairwise distinct opacities 0.1 ... 0.9 in depth order, sigma 1.2 ... 2.2 px, spread over the tile
    so that T stays above 1e-4 everywhere: every one of them is staged and reduced, 4 per flush -- 1 and 3 leave a partial flush,
    4 a full one, 5 a full and a partial one, 64 a whole batch, 65 a batch boundary.  An opacity taken from another staged
    instance multiplies a row's five geometric words by another row's opacity."""
    rng = np.random.RandomState(100 + n)
    opac = np.linspace(0.1, 0.9, n) if n > 1 else np.array([0.5])
    opac = opac[rng.permutation(n)]
    px, py = 1.0 + 14.0 * rng.rand(n), 1.0 + 14.0 * rng.rand(n)
    scene = gr._scene(px, py, np.linspace(3.5, 4.5, n), rng.randint(4, 8, size=n).astype(np.float64), opac, 16, 16, FOVX, seed=83)
    return scene, gsr_scene.make_camera(16, 16, fovx=FOVX)
