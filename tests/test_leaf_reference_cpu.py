"""CPU: the float64 reference of the leaf-activation backward (tests/torch_leaf.py) against torch.autograd, and the conditions that
tests/test_gaussian_pass_gpu.py relies on in its two fixtures, checked with the CPU oracle on the activated values."""
import numpy as np
import torch

import gsr_scene
import torch_leaf as tl
import util

W, H = 128, 96
GSR_SLOT_COOP = 30   # csrc/gsr_internal.h: longer runs of gradient slots are summed by the whole wave


def _oracle(leaves, D=3):
    act = tl.activated(leaves)
    scene = gsr_scene.Scene(act["means3D"], act["scales"], act["rotations"], act["opacities"], act["shs"], torch.tensor([0.1, 0.2, 0.3]))
    cam = gsr_scene.make_camera(W, H)
    o = util.oracle_forward(scene, cam, D)
    return o, util.oracle.backward(o, tl.upstream(W, H).numpy())


def test_reference_agrees_with_autograd_in_float64():
    leaves = tl.fixture_a()
    g = torch.Generator().manual_seed(3)
    gs = [torch.randn(t.shape, generator=g) * 10.0 ** torch.randint(-6, 3, (t.shape[0], 1), generator=g) for t in leaves[3:]]
    ref, auto = tl.reference(*leaves[3:], *gs), tl.autograd_reference(*leaves[3:], *gs)
    for k in ref:
        # relative to the row's own magnitude: rows differ by many orders
        scale = auto[k].abs().amax(dim=1, keepdim=True).clamp_min(1e-300)
        err = float(((ref[k] - auto[k]).abs() / scale).max())
        assert err <= 1e-12, (k, err)
    # the zero quaternion: g / 1e-12, nothing from q
    assert torch.equal(ref["rotation"][tl.ROW_ZERO_QUAT], gs[2][tl.ROW_ZERO_QUAT].double() / 1e-12)
    # (c) of the reference itself is zero, of the stock chain small but not zero, and a wrong factor is seen
    e = tl.normalised_error(ref, ref, *leaves[3:], *gs)
    assert all(float(v.max()) == 0.0 for v in e.values())
    st = tl.stock(*leaves[3:], *gs)
    e = tl.normalised_error(st, ref, *leaves[3:], *gs)
    sel = leaves[3][:, 0].abs() <= 8
    assert 0 < float(e["opacity"][sel].max()) < 1e-3 and 0 < float(e["scaling"].max()) < 1e-6 and 0 < float(e["rotation"].max()) < 1e-5
    wrong = dict(st, opacity=gs[0] * torch.sigmoid(leaves[3]))
    assert float(tl.normalised_error(wrong, ref, *leaves[3:], *gs)["opacity"][sel].max()) > 0.5


def test_fixture_a_holds_its_conditions():
    leaves = tl.fixture_a()
    xyz, dc, fr, opacity, scaling, rotation = leaves
    P = xyz.shape[0]
    assert P == 257 and fr.shape == (P, 15, 3)
    l = opacity[:, 0]
    for lo, hi in tl.BANDS:
        n = int(((l.abs() >= lo) & (l.abs() <= hi)).sum())
        assert 70 <= n <= 100, (lo, hi, n)
    assert float(l[tl.ROW_LOGIT_PLUS20]) == 20.0 and float(l[tl.ROW_LOGIT_MINUS20]) == -20.0
    assert float(torch.sigmoid(l[tl.ROW_LOGIT_PLUS20])) == 1.0
    assert float(scaling.min()) >= -9.0 and float(scaling.max()) <= 1.0
    assert float((scaling.amax(dim=1) - scaling.amin(dim=1)).median()) > 1.0    # mixed within a Gaussian
    n = rotation.norm(dim=1)
    assert bool((rotation[tl.ROW_ZERO_QUAT] == 0).all()) and abs(float(n[tl.ROW_UNIT_QUAT]) - 1.0) <= 2.0 ** -23
    rest = torch.ones(P, dtype=torch.bool)
    rest[[tl.ROW_ZERO_QUAT, tl.ROW_UNIT_QUAT]] = False
    assert 1e-3 <= float(n[rest].min()) < 1e-2 and 1e2 < float(n[rest].max()) <= 1e3

    o, og = _oracle(leaves)
    vis = o["radii"] > 0
    assert vis.mean() >= 0.6 and vis[P - 1] and (~vis).sum() >= 20
    assert vis[[tl.ROW_ZERO_QUAT, tl.ROW_UNIT_QUAT, tl.ROW_LOGIT_PLUS20, tl.ROW_LOGIT_MINUS20, tl.ROW_BIG]].all()
    assert o["tiles_touched"][tl.ROW_BIG] > GSR_SLOT_COOP and (o["tiles_touched"][vis] <= GSR_SLOT_COOP).sum() > 100
    live = vis & (og["dL_dopacity"][:, 0] != 0)
    for lo, hi in tl.BANDS:
        n = int((live & (l.abs().numpy() >= lo) & (l.abs().numpy() <= hi)).sum())
        assert n >= 10, (lo, hi, n)
    # the named rows take part: the zero quaternion and the +20 logit have a gradient to carry through the activation
    assert live[tl.ROW_ZERO_QUAT] and live[tl.ROW_LOGIT_PLUS20] and live[P - 1]
    assert np.abs(og["dL_dscales"][tl.ROW_ZERO_QUAT]).max() > 0
    # ... but every term of dL/dq of the covariance carries a component of q (backward.cu:281-345), so at q = 0 the gradient that
    # reaches the normalisation is exactly zero: what the GPU test pins on that row is a finite, exactly zero result
    assert np.abs(og["dL_drotations"][tl.ROW_ZERO_QUAT]).max() == 0 and np.abs(og["dL_drotations"][tl.ROW_UNIT_QUAT]).max() > 0
    # the two smaller layouts of A2 see the same geometry
    for D, M in ((2, 9), (0, 1)):
        o2, _ = _oracle([xyz, dc, fr[:, :M - 1], opacity, scaling, rotation], D)
        assert np.array_equal(o2["radii"], o["radii"])


def test_fixture_b_holds_its_conditions():
    leaves = tl.fixture_b()
    P = leaves[0].shape[0]
    assert P == 333 and tl.PARTS_B[-1][0] + tl.PARTS_B[-1][1] == P
    o, _ = _oracle(leaves)
    vis = o["radii"] > 0
    for first, count in tl.PARTS_B:
        assert first % 64 == 0
        v = vis[first:first + count]
        if count == 1:
            assert v[0] and first == 64
        else:
            assert v.sum() >= 8 and (~v).sum() >= 2, (first, count, int(v.sum()))
    assert (tl.PARTS_B[1][0] // 64) % 2 == 1 and P % 64 != 0   # (64, 1) starts at an odd multiple of 64; the last part ends in mid-wave
