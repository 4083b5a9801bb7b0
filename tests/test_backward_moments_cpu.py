"""CPU: the scenes of tests/moment_scenes.py are what tests/test_backward_moments_gpu.py takes them for, from the oracle alone: the
per-row bound is not vacuous on them (grad_rows.cap_shares >= CAP_SHARE at CAP in every blend tensor), every Gaussian has terms,
and the geometry each scene is named after is there."""
import numpy as np
import pytest

import grad_rows as gr
import moment_scenes as ms
import util


def _budget(scene, cam, ramp=0.0):
    o = util.oracle_forward(scene, cam, 0)
    dpix = gr.smooth_dpix(o, cam, ramp=ramp)
    return o, util.oracle.blend_backward_budget(o, dpix.numpy())


def _not_vacuous(bud, label):
    shares = gr.cap_shares(bud)
    print(f"[{label}] share of rows with E <= {gr.CAP} |S|: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    for k, v in shares.items():
        assert v >= gr.CAP_SHARE, (label, k, v)


@pytest.mark.parametrize("name", ["centre", "left", "needle"])
def test_single_gaussian(name):
    scene, cam, ramp = ms.single(name)
    o, bud = _budget(scene, cam, ramp)
    assert o["num_rendered"] == 1 and bud["n"][0] >= 16
    _not_vacuous(bud, name)
    mx = float(o["means2D"][0, 0])
    if name == "centre":
        assert 1 < mx < 15
    if name == "left":
        assert -44 < mx < -40, mx   # every pixel of the tile lies to its right
    if name == "needle":
        a, b, c = (float(v) for v in o["conic_opacity"][0, :3])
        assert abs(b) > 0.9 * np.sqrt(a * c) and 0.99 < a / c < 1.01, (a, b, c)   # thin, and diagonal


def test_odd_image():
    scene, cam = ms.odd_image()
    o, bud = _budget(scene, cam)
    assert (o["W"], o["H"]) == (17, 33)
    _not_vacuous(bud, "17 x 33")
    rows = ms.rows_hit(o, 17, 33)
    assert sum(1 for r in rows if len(r) and r.max() == 32) >= 2, "nothing reaches the one-pixel tile row"
    assert (bud["n"] > 0).sum() >= 30


def test_one_band():
    scene, cam = ms.one_band()
    o, bud = _budget(scene, cam)
    assert o["num_rendered"] == 8 and (bud["n"] > 0).all()
    _not_vacuous(bud, "one band")
    bands = [sorted({int(r) // 4 for r in rows}) for rows in ms.rows_hit(o, 16, 16)]
    assert bands == [[0], [0], [1], [1], [2], [2], [3], [3]], bands


@pytest.mark.parametrize("n", ms.ONE_TILE_COUNTS)
def test_one_tile(n):
    scene, cam = ms.one_tile(n)
    o, bud = _budget(scene, cam)
    assert o["num_rendered"] == n and (bud["n"] > 0).all(), "a Gaussian without a term: not every instance is reduced"
    assert len(np.unique(scene.opacities.numpy())) == n
    assert o["n_contrib"].max() <= n
    _not_vacuous(bud, f"one tile, {n}")
