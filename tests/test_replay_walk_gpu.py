"""GPU: list lengths at the batch edges of the replay walk (csrc/gsr_replay.h) -- the one place contrib.hip, features.hip,
distortion.hip and median.hip now take their tile walk from.  The walk stages 64 instances per batch, fetches records one batch ahead
and ids two batches ahead; the scenes of the four passes' own tests have long lists, none pins a list that ends at, just before or just
after a batch.

Scenes: N in {1, 63, 64, 65, 128, 129} small Gaussians of opacity 0.02 whose footprints lie inside tile (1, 0) of a 37 x 21 image
(3 x 2 tiles, ragged on the right and at the bottom); the other five tiles are empty (a walk of length 0).  No pixel saturates
(0.98^129 = 0.07), so the tile's list is walked whole: its range length is asserted to be exactly N.

References are the existing ones: the colour passes bit for bit (test_features_gpu.py), the full-walk twin of the median forward bit
for bit (test_median_gpu.py), the float64 walk of test_contrib_gpu.py, and float64 autograd through tests/torch_splat_feat.py,
torch_splat_dist.py and torch_splat_median.py with test_autograd_cpu.py's bars as those tests carry them.  Pixels whose accept /
reject decisions sit within the oracle's margin (and, for the median, whose choice is ambiguous) are masked out of the losses as
there, their share capped at 5 % as there."""
import functools

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
import gsr_scene
import util
import test_contrib_gpu as tc
import test_distortion_gpu as td
import test_features_gpu as tf
import test_median_gpu as tm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = (1, 63, 64, 65, 128, 129)
W, H, D, K = 37, 21, 1, 5
TILE = 1   # tile (tx = 1, ty = 0): pixels x 16..31, y 0..15


@functools.lru_cache(maxsize=None)
def _scene(N, opacity=0.02):
    """N Gaussians of one opacity whose centres project to x in [21.5, 26.5], y in [5.5, 10.5] with a screen-space sigma of at most 1.1 pixels: the
    3 sigma footprint (4 pixels at most) stays inside the tile."""
    cam = gsr_scene.make_camera(W, H)
    g = torch.Generator().manual_seed(100 + N)
    focal = W / (2.0 * cam.tanfovx)
    z = 4.0 + (torch.rand(N, generator=g) * 0.8 - 0.4)   # view depth; the camera sits at (0, 0, -4)
    px, py = 21.5 + 5.0 * torch.rand(N, generator=g), 5.5 + 5.0 * torch.rand(N, generator=g)
    means = torch.stack([(px + 0.5 - W / 2.0) / focal * z, (py + 0.5 - H / 2.0) / focal * z, z - 4.0], 1)
    sigma = 0.6 + 0.4 * torch.rand(N, 3, generator=g)    # pixels, before the 0.3 dilation
    scales = sigma * (z / focal)[:, None]
    rot = torch.nn.functional.normalize(torch.randn(N, 4, generator=g), dim=1)
    shs = torch.randn(N, (D + 1) ** 2, 3, generator=g)
    shs[:, 1:, :] *= 0.2
    scene = gsr_scene.Scene(means.contiguous(), scales.contiguous(), rot.contiguous(), torch.full((N, 1), opacity), shs.contiguous(),
                            torch.tensor([0.1, 0.2, 0.3]))
    return scene, cam


def _check_ranges(scene, cam, N):
    rng = tf._ranges(scene, cam, D)
    lens = (rng[:, 1] - rng[:, 0]).cpu().tolist()
    assert len(lens) == 6 and lens[TILE] == N and sum(lens) == N, (N, lens)


@functools.lru_cache(maxsize=None)
def _oracle(N):
    """The CPU oracle's state of the scene and the mask of the pixels no test below excludes; the share of excluded ones is capped."""
    scene, cam = _scene(N)
    o = util.oracle_forward(scene, cam, D, margin=1e-3)
    ok = torch.from_numpy((o["fragile"] == 0).reshape(H, W))
    share = float((~ok).float().mean())
    print(f"replay walk N={N}: fragile share {share:.4f}")
    assert share <= 0.05, (N, share)
    return o, ok


def _leaf64(scene):
    leaf = lambda x: x.double().clone().requires_grad_(True)
    return dict(means3D=leaf(scene.means3D), scales=leaf(scene.scales), rotations=leaf(scene.rotations), opacities=leaf(scene.opacities),
                shs=leaf(scene.shs))


def _check_bars(label, grads, ref, bars):
    for n, bar in bars.items():
        e = tf._nerr(grads[n].cpu().reshape(ref[n].shape), ref[n])
        line = f"replay walk {label} dL/d{n}: err {e:.2e} bar {bar:.2e}"
        print(line)
        util.parity_log(line)
        assert e < bar, (label, n, e, bar)


# ---- (a) the feature forward has the colour passes' bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_feature_forward_equals_colour_passes_bit_for_bit(N):
    scene, cam = _scene(N)
    _check_ranges(scene, cam, N)
    feats = tf._feats(N, K)
    r = tf.fused(scene, cam, D, feats, None, backward=False)
    f = feats.to(DEV)
    zero = torch.zeros(3, device=DEV)
    for k0 in range(0, K, 3):
        n = min(3, K - k0)
        cols = torch.cat([f[:, k0:k0 + n], torch.zeros(N, 3 - n, device=DEV)], 1).contiguous()
        out_color = tf._state(scene, cam, D, colors=cols, bg=zero)[1]
        for c in range(n):
            assert torch.equal(r["fmap"][k0 + c], out_color[c]), (N, k0 + c)
    assert float(r["fmap"].abs().max()) > 0
    outside = torch.ones(H, W, dtype=torch.bool)
    outside[0:16, 16:32] = False
    assert float(r["fmap"][:, outside.to(DEV)].abs().max()) == 0.0   # the empty tiles are written, with zeros


# ---- (b) the median forward's early exit changes nothing -----------------------------------------------------------------------------------
# At opacity 0.02 T stays high and the exit comes from n_contrib; at 0.3 the same footprints take T below 0.5 (asserted on the
# alpha map for the lists of 63 and more), where the T-based stop decides.
@pytest.mark.parametrize("opacity", [0.02, 0.3])
@pytest.mark.parametrize("N", SIZES)
def test_median_exit_twin_equals_the_full_walk(N, opacity):
    from diff_gaussian_rasterization import _C
    scene, cam = _scene(N, opacity)
    a = tm.direct(scene, cam, D, "depth")
    b = tm.direct(scene, cam, D, "depth", median_debug=_C.DEBUG_MEDIAN_FULL_WALK)
    assert int((a["mi"] >= 0).sum()) > 0
    if opacity == 0.3 and N >= 63:
        assert float(a["alpha"].max()) > 0.5
    for k in ("med", "state", "mi", "di", "dw"):
        assert torch.equal(a[k], b[k]), (N, k)


# ---- (c) float64 references ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_feature_gradients_match_float64_autograd(N):
    import torch_splat_feat
    scene, cam = _scene(N)
    o, ok = _oracle(N)
    feats = tf._feats(N, K)
    g = torch.Generator().manual_seed(4)
    dpix, dmap = torch.randn(3, H, W, generator=g) * ok, torch.randn(K, H, W, generator=g) * ok
    t = _leaf64(scene)
    t["features"] = feats.double().clone().requires_grad_(True)
    img, fmap = torch_splat_feat.render(o, t["means3D"], t["scales"], t["rotations"], t["opacities"], t["shs"], t["features"])
    ((img * dpix.double()).sum() + (fmap * dmap.double()).sum()).backward()
    z = torch.zeros(1, H, W, device=DEV)
    f = tf.fused(scene, cam, D, feats, (dpix.to(DEV), dmap.to(DEV), z, z))
    okn = ok.numpy()
    assert np.abs(fmap.detach().numpy() - f["fmap"].cpu().numpy())[:, okn].max() < 5e-5 * max(1.0, float(fmap.detach().abs().max()))
    _check_bars(f"features N={N}", f["grads"], {n: v.grad for n, v in t.items()}, tf.AUTOGRAD_BARS)
    # the features-only backward (into_slots = 0, the kernel's other instantiation) on the same state: the same bits
    from diff_gaussian_rasterization import _C
    R, _, _, geom, binning, img = tf._state(scene, cam, D)
    only = _C.features_backward_only(geom, binning, img, R, N, W, H, feats.to(DEV), dmap.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(only, f["grads"]["features"]), N


@pytest.mark.parametrize("N", SIZES)
def test_distortion_gradients_match_float64_autograd(N):
    import torch_splat_dist
    scene, cam = _scene(N)
    o, ok = _oracle(N)
    g = torch.Generator().manual_seed(4)
    dpix, gd = torch.randn(3, H, W, generator=g) * ok, torch.randn(1, H, W, generator=g) * ok
    t = _leaf64(scene)
    img, _, _, dist = torch_splat_dist.render(o, t["means3D"], t["scales"], t["rotations"], t["opacities"], t["shs"], "depth")
    ((img * dpix.double()).sum() + (dist * gd[0].double()).sum()).backward()
    ref = {n: v.grad for n, v in t.items()}
    with torch.no_grad():
        d32 = torch_splat_dist.render(o, scene.means3D, scene.scales, scene.rotations, scene.opacities, scene.shs, "depth",
                                      dtype=torch.float32)[3].double()
    res = {torch.float64: dist.detach(), torch.float32: d32}
    e32 = float((res[torch.float32] - res[torch.float64]).abs().max())
    z = torch.zeros(1, H, W, device=DEV)
    f = td.fused(scene, cam, D, "depth", (dpix.to(DEV), gd.to(DEV), z, z))
    err = float((f["dist"][0].cpu().double() - res[torch.float64]).abs()[ok].max())
    print(f"replay walk distortion N={N}: map vs float64 {err:.3e} (fp32 restatement {e32:.3e})")
    if N == 1:   # one Gaussian: Dist = 0 exactly, on both sides
        assert float(f["dist"].abs().max()) == 0.0 and e32 == 0.0
    else:
        assert err <= 10 * e32, (err, e32)
    _check_bars(f"distortion N={N}", f["grads"], ref, td.AUTOGRAD_BARS)


@pytest.mark.parametrize("N", SIZES)
def test_median_gradients_match_float64_autograd(N):
    import torch_splat_median
    scene, cam = _scene(N)
    o, ok = _oracle(N)
    g = torch.Generator().manual_seed(6)
    dpix, gm = torch.randn(3, H, W, generator=g), torch.randn(1, H, W, generator=g)
    t = _leaf64(scene)
    img, _, _, med, maps = torch_splat_median.render(o, t["means3D"], t["scales"], t["rotations"], t["opacities"], t["shs"], "depth")
    ok = ok & ~maps["ambiguous"]
    share = float((~ok).float().mean())
    print(f"replay walk median N={N}: excluded share {share:.4f}")
    assert share <= 0.05, share
    dpix, gm = dpix * ok, gm * ok
    ((img * dpix.double()).sum() + (med * gm[0].double()).sum()).backward()
    z = torch.zeros(1, H, W, device=DEV)
    f = tm.fused(scene, cam, D, "depth", (dpix.to(DEV), gm.to(DEV), z, z, z))
    assert bool((f["mi"].cpu().long() == maps["median_index"])[ok].all())
    assert bool((f["di"].cpu().long() == maps["dominant_index"])[ok].all())
    _check_bars(f"median N={N}", f["grads"], {n: v.grad for n, v in t.items()}, tm.AUTOGRAD_BARS)


@pytest.mark.parametrize("N", SIZES)
def test_contributions_match_the_float64_walk(N):
    scene, cam = _scene(N)
    r, inp = tc._forward(scene, cam)
    torch.cuda.synchronize()
    st = util.unpack_state(dict(R=r[0], geom=r[3], binning=r[4], img=r[5]), N, W, H)
    lens = st["ranges"].astype(np.int64)
    assert int(lens[TILE, 1] - lens[TILE, 0]) == N
    m = tc._weight_map(W, H)
    tc._check_against(tc.ref_walk(st, W, H), tc._contrib(r, N, cam), W * H, f"replay walk contrib N={N} m=1")
    tc._check_against(tc.ref_walk(st, W, H, m.numpy()), tc._contrib(r, N, cam, m.to(DEV)), W * H, f"replay walk contrib N={N} map")
