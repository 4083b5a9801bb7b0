"""GPU: depth and alpha maps from the same blend pass (GaussianRasterizer(..., depth_alpha="depth" | "invdepth"),
include/gsr.h gsr_aux_args).

D(p) = sum_i v_i alpha_i T_i(p) over the pairs that blend into the colour (v_i = view-space z_i, or 1 / z_i), A(p) = 1 - T_final(p).
The reference side of every check is the two-pass composition through the existing rasterizer: the image pass, plus an aux
pass with colors_precomp = stack(v, 1, 0) and a zero background, v computed in torch from means3D and the view matrix (so
autograd chains dL/dz), fed dL/dpix = (dL/dD, dL/dA, 0).  Both passes take the HIP kernels' decisions, so no pixel is excluded."""
import numpy as np
import pytest
import torch

import gsr_scene
import util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("means3D", "means2D", "shs", "opacities", "scales", "rotations")
LEAF_NAMES = ("xyz", "means2D", "features_dc", "features_rest", "opacity", "scaling", "rotation")


def _v(means, viewmatrix, mode):
    z = means @ viewmatrix[:3, 2] + viewmatrix[3, 2]   # the z row of the column-major view matrix (gsr_transform_point_4x3)
    return z if mode == "depth" else 1.0 / z


def _maps(seed, H, W):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(3, H, W, generator=g).to(DEV), torch.randn(1, H, W, generator=g).to(DEV),
            torch.randn(1, H, W, generator=g).to(DEV))


def _leaves(scene):
    return {"means3D": scene.means3D.to(DEV).clone().requires_grad_(True),
            "means2D": torch.zeros(scene.means3D.shape, device=DEV, requires_grad=True),
            "shs": scene.shs.to(DEV).clone().requires_grad_(True),
            "opacities": scene.opacities.to(DEV).clone().requires_grad_(True),
            "scales": scene.scales.to(DEV).clone().requires_grad_(True),
            "rotations": scene.rotations.to(DEV).clone().requires_grad_(True)}


def _grads(t, names):
    return {n: (t[n].grad.clone() if t[n].grad is not None else torch.zeros_like(t[n])) for n in names}


def fused(scene, cam, D, mode, dpix, dD, dA, debug=False, backward=True):
    """-> (color, radii, depth, alpha, grads) through GaussianRasterizer(depth_alpha=mode)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    st = util.hip_settings(scene, cam, D, DEV, debug=debug)
    t = _leaves(scene)
    color, radii, depth, alpha = GaussianRasterizer(st, depth_alpha=mode)(
        means3D=t["means3D"], means2D=t["means2D"], shs=t["shs"], opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])
    if not backward:
        return color.detach(), radii, depth.detach(), alpha.detach(), None
    loss = (color * dpix).sum()
    if dD is not None:
        loss = loss + (depth * dD).sum()
    if dA is not None:
        loss = loss + (alpha * dA).sum()
    loss.backward()
    torch.cuda.synchronize()
    return color.detach(), radii, depth.detach(), alpha.detach(), _grads(t, NAMES)


def two_pass(scene, cam, D, mode, dpix, dD, dA, debug=False, split=False):
    """-> (color, radii, aux image (3,H,W), grads) of the image pass + the aux pass.  split: the image pass's dL/dpix cut into
    two random parts, each with a pass of its own -- the same gradients mathematically, with part of what one pass sums BEFORE
    the per-Gaussian chain summed AFTER it, as the two-pass composition does with the image and aux terms: check_grads'
    reproducibility band."""
    from diff_gaussian_rasterization import GaussianRasterizer
    st = util.hip_settings(scene, cam, D, DEV, debug=debug)
    st0 = st._replace(bg=torch.zeros(3, device=DEV))
    t = _leaves(scene)
    color, radii = GaussianRasterizer(st)(means3D=t["means3D"], means2D=t["means2D"], shs=t["shs"], opacities=t["opacities"],
                                          scales=t["scales"], rotations=t["rotations"])
    v = _v(t["means3D"], st.viewmatrix, mode)
    cols = torch.stack([v, torch.ones_like(v), torch.zeros_like(v)], dim=1)
    aux, _ = GaussianRasterizer(st0)(means3D=t["means3D"], means2D=t["means2D"], colors_precomp=cols, opacities=t["opacities"],
                                     scales=t["scales"], rotations=t["rotations"])
    H, W = cam.image_height, cam.image_width
    z = torch.zeros(1, H, W, device=DEV)
    daux = torch.cat([dD if dD is not None else z, dA if dA is not None else z, z], 0)
    if split:
        part = torch.randn(dpix.shape, generator=torch.Generator().manual_seed(99)).to(DEV)
        c2, _ = GaussianRasterizer(st)(means3D=t["means3D"], means2D=t["means2D"], shs=t["shs"], opacities=t["opacities"],
                                       scales=t["scales"], rotations=t["rotations"])
        loss = (color * part).sum() + (c2 * (dpix - part)).sum()
    else:
        loss = (color * dpix).sum()
    (loss + (aux * daux).sum()).backward()
    torch.cuda.synchronize()
    return color.detach(), radii, aux.detach(), _grads(t, NAMES)


def check_forward(f, r):
    color, radii, depth, alpha, _ = f
    rc, rr, aux, _ = r
    assert torch.equal(color, rc) and torch.equal(radii, rr)
    d = float((depth[0] - aux[0]).abs().max())
    assert d <= 1e-6 * max(float(aux[0].abs().max()), 1e-30), f"depth err {d}"
    a = float((alpha[0] - aux[1]).abs().max())
    assert a <= 1e-5, f"alpha err {a}"


def _nerr(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-30)


CHAIN = ("scales", "rotations", "scaling", "rotation")


def check_grads(g, rg, band=None, label=""):
    """The repository's end-to-end bar (test_parity_gpu.py): 1e-5 of the largest element -- for every gradient but the scale /
    quaternion ones.  The conic -> covariance -> scale / quaternion chain amplifies last-bit differences of dL/dconic (its
    determinant terms cancel for needle-shaped splats), and one pass sums the colour and aux terms before that chain where the
    two passes sum them after it; there the bar is the reference side's own reproducibility band, measured per case as the
    distance between two exact compositions that differ only in that order (two_pass(split=True)).  One random split is one
    sample of the band (measured: the fused result sits 2 ... 7 of them away, 1e-5 ... 3e-4 of the largest element), so the bar
    is max(5e-5 -- test_boundary_gpu.py's split-vs-unsplit bar for the same chain --, 10 x the sample)."""
    for n in rg:
        e = _nerr(g[n], rg[n])
        b = max(5e-5, 10.0 * _nerr(band[n], rg[n])) if (band is not None and n in CHAIN) else 1e-5
        print(f"{label} {n}: {e:.2e} (bar {b:.2e})")
        assert e <= b, (label, n, e, b)


def _state(scene, cam, D, mode, debug=0):
    """Direct binding calls: default and aux forward states side by side."""
    from diff_gaussian_rasterization import _C
    st = util.hip_settings(scene, cam, D, DEV)
    e = torch.empty(0, device=DEV)
    t = {k: getattr(scene, k).to(DEV) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    args = (st.bg, t["means3D"], e, t["opacities"], t["scales"], t["rotations"], 1.0, e, st.viewmatrix, st.projmatrix, st.tanfovx,
            st.tanfovy, st.image_height, st.image_width, t["shs"], D, st.campos, False, debug)
    a = _C.rasterize_gaussians(*args)
    b = _C.rasterize_gaussians_depth_alpha(mode, *args)
    torch.cuda.synchronize()
    return a, b


def _same_state(a, b, P, W, H):
    from diff_gaussian_rasterization import _C
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    il = _C.image_layout(W, H)
    N, T = W * H, ((W + 15) // 16) * ((H + 15) // 16)
    for off, n in ((il.final_T, 4 * N), (il.n_contrib, 4 * N), (il.ranges, 8 * T), (il.tile_max_contrib, 4 * T)):
        assert torch.equal(a[5][off:off + n], b[5][off:off + n])
    gl = _C.geometry_layout(P)
    sa = a[3][gl.splat:gl.splat + 48 * P].view(torch.int32).view(P, 12)
    sb = b[3][gl.splat:gl.splat + 48 * P].view(torch.int32).view(P, 12)
    vis = a[2] > 0
    assert torch.equal(sa[vis, :11], sb[vis, :11])   # the record but its last word (v)
    for name, size in (("depth_keys", 4), ("tiles_touched", 4), ("rect", 8), ("slot_base", 4)):
        off = getattr(gl, name)
        assert torch.equal(a[3][off:off + size * P], b[3][off:off + size * P]), name
    R = a[0]
    if R:
        bl = _C.binning_layout(P, R, W, H)
        rng = a[5][il.ranges:il.ranges + 8 * T].view(torch.int32).view(T, 2)
        L = int(rng[:, 1].max())
        assert torch.equal(a[4][bl.point_list:bl.point_list + 4 * L], b[4][bl.point_list:bl.point_list + 4 * L])
    alpha = b[7][0]
    final_T = b[5][il.final_T:il.final_T + 4 * N].view(torch.float32).view(H, W)
    assert torch.equal(alpha, 1 - final_T)


def _c1():
    return gsr_scene.make_scene(10_000, -3.5, sh_degree=3, seed=5), gsr_scene.make_camera(256, 256), 3


def _heavy():
    from test_boundary_gpu import _heavy_scene
    return _heavy_scene()


CASES = {"C1": _c1, "C2": lambda: gsr_scene.make_config("C2", seed=2), "C3": lambda: gsr_scene.make_config("C3", seed=3),
         "heavy": _heavy}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("mode", ["depth", "invdepth"])
def test_forward_and_backward_match_two_passes(case, mode):
    scene, cam, D = CASES[case]()
    P, W, H = scene.means3D.shape[0], cam.image_width, cam.image_height
    a, b = _state(scene, cam, D, mode)
    _same_state(a, b, P, W, H)
    dpix, dD, dA = _maps(11, H, W)
    f = fused(scene, cam, D, mode, dpix, dD, dA)
    r = two_pass(scene, cam, D, mode, dpix, dD, dA)
    check_forward(f, r)
    check_grads(f[4], r[3], two_pass(scene, cam, D, mode, dpix, dD, dA, split=True)[3], label=f"{case}/{mode}")


@pytest.mark.parametrize("which", ["depth_only", "alpha_only"])
def test_one_aux_gradient(which):
    scene, cam, D = _heavy()
    H, W = cam.image_height, cam.image_width
    dpix, dD, dA = _maps(12, H, W)
    dD, dA = (dD, None) if which == "depth_only" else (None, dA)
    f = fused(scene, cam, D, "depth", dpix, dD, dA)
    r = two_pass(scene, cam, D, "depth", dpix, dD, dA)
    check_forward(f, r)
    check_grads(f[4], r[3], two_pass(scene, cam, D, "depth", dpix, dD, dA, split=True)[3], label=which)


def test_heavy_scene_takes_band_splits_and_depth_segments():
    """The skewed scene must exercise both splits on the aux path: band entries in the forward's dispatch list, depth
    segments (lists >= 2 x GSR_CKPT_STRIDE) in the backward's."""
    from diff_gaussian_rasterization import _C
    scene, cam, D = _heavy()
    W, H = cam.image_width, cam.image_height
    T = ((W + 15) // 16) * ((H + 15) // 16)
    _, b = _state(scene, cam, D, "depth")
    R, color, radii, geom, binning, img, depth, alpha, auxbuf = b
    il = _C.image_layout(W, H)

    def entries(count):
        v = img[il.tile_order:il.tile_order + 4 * count].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        return v[v != 0xFFFFFFFF]
    assert int(((entries(T + 3 * min(2048, T // 4)) >> 28) > 0).sum()) >= 4, "no tile was split into bands"
    rng = img[il.ranges:il.ranges + 8 * T].view(torch.int32).view(T, 2)
    assert int((rng[:, 1] - rng[:, 0]).max()) >= 2 * 512, "no list of two checkpoint strides"
    st = util.hip_settings(scene, cam, D, DEV)
    e = torch.empty(0, device=DEV)
    t = {k: getattr(scene, k).to(DEV) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    dpix, dD, dA = _maps(13, H, W)
    _C.rasterize_gaussians_backward_depth_alpha("depth", st.bg, t["means3D"], radii, e, t["scales"], t["rotations"], 1.0, e,
                                                st.viewmatrix, st.projmatrix, st.tanfovx, st.tanfovy, dpix, t["shs"], D, st.campos,
                                                geom, R, binning, img, auxbuf, dD[0], dA[0], False)
    torch.cuda.synchronize()
    assert int(((entries(T + min(4096, T // 2)) >> 28) > 0).sum()) >= 1, "no tile was cut into depth segments"


def test_c5_size_radix_depth_path():
    scene, cam, D = gsr_scene.make_config("C5", seed=4)
    assert scene.means3D.shape[0] > (2 << 20)   # beyond the bucket depth sort: the global radix passes
    dpix, dD, dA = _maps(14, cam.image_height, cam.image_width)
    f = fused(scene, cam, D, "depth", dpix, dD, dA)
    r = two_pass(scene, cam, D, "depth", dpix, dD, dA)
    check_forward(f, r)
    check_grads(f[4], r[3], two_pass(scene, cam, D, "depth", dpix, dD, dA, split=True)[3], label="C5")


def _leaf_params(scene):
    dc = scene.shs[:, :1, :].contiguous()
    rest = scene.shs[:, 1:, :].contiguous()
    g = torch.Generator().manual_seed(3)
    raw_rot = scene.rotations * (0.5 + torch.rand(scene.rotations.shape[0], 1, generator=g))
    return {"xyz": scene.means3D, "features_dc": dc, "features_rest": rest, "opacity": torch.logit(scene.opacities),
            "scaling": torch.log(scene.scales), "rotation": raw_rot}


@pytest.mark.parametrize("mode", ["depth", "invdepth"])
def test_leaf_parameters(mode):
    from diff_gaussian_rasterization import GaussianRasterizer
    from fused_params import rasterize_leaf_gaussians
    scene, cam, D = _heavy()
    H, W = cam.image_height, cam.image_width
    dpix, dD, dA = _maps(15, H, W)
    lp = _leaf_params(scene)
    st = util.hip_settings(scene, cam, D, DEV)

    def leaves():
        t = {k: v.to(DEV).clone().requires_grad_(True) for k, v in lp.items()}
        t["means2D"] = torch.zeros(scene.means3D.shape, device=DEV, requires_grad=True)
        return t
    t = leaves()
    color, radii, depth, alpha = rasterize_leaf_gaussians(t["xyz"], t["means2D"], t["features_dc"], t["features_rest"], t["opacity"],
                                                          t["scaling"], t["rotation"], st, depth_alpha=mode)
    ((color * dpix).sum() + (depth * dD).sum() + (alpha * dA).sum()).backward()
    g = _grads(t, LEAF_NAMES)
    u = leaves()
    act = dict(means3D=u["xyz"], means2D=u["means2D"], shs=torch.cat([u["features_dc"], u["features_rest"]], 1),
               opacities=torch.sigmoid(u["opacity"]), scales=torch.exp(u["scaling"]),
               rotations=torch.nn.functional.normalize(u["rotation"]))
    rc, rr = GaussianRasterizer(st)(**act)
    v = _v(u["xyz"], st.viewmatrix, mode)
    cols = torch.stack([v, torch.ones_like(v), torch.zeros_like(v)], 1)
    act0 = dict(act, colors_precomp=cols)
    del act0["shs"]
    black = GaussianRasterizer(st._replace(bg=torch.zeros(3, device=DEV)))
    aux, _ = black(**act0)
    daux = torch.cat([dD, dA, torch.zeros_like(dD)], 0)
    ((rc * dpix).sum() + (aux * daux).sum()).backward()
    torch.cuda.synchronize()
    check_forward((color.detach(), radii, depth.detach(), alpha.detach(), None), (rc.detach(), rr, aux.detach(), None))
    ref = _grads(u, LEAF_NAMES)
    w = leaves()   # the band: the image pass's dL/dpix in two parts (two_pass(split=True))
    act = dict(means3D=w["xyz"], means2D=w["means2D"], opacities=torch.sigmoid(w["opacity"]), scales=torch.exp(w["scaling"]),
               rotations=torch.nn.functional.normalize(w["rotation"]))
    shs = torch.cat([w["features_dc"], w["features_rest"]], 1)
    part = torch.randn(dpix.shape, generator=torch.Generator().manual_seed(99)).to(DEV)
    loss = (GaussianRasterizer(st)(shs=shs, **act)[0] * part).sum() + (GaussianRasterizer(st)(shs=shs, **act)[0] * (dpix - part)).sum()
    v = _v(w["xyz"], st.viewmatrix, mode)
    loss = loss + (black(colors_precomp=torch.stack([v, torch.ones_like(v), torch.zeros_like(v)], 1), **act)[0] * daux).sum()
    loss.backward()
    check_grads(g, ref, _grads(w, LEAF_NAMES), label=f"leaf/{mode}")


def test_zero_aux_gradients_equal_default_backward():
    """Explicit all-zero dL/dD and dL/dA run the aux kernels; every gradient must equal the default backward's."""
    from diff_gaussian_rasterization import GaussianRasterizer
    scene, cam, D = _heavy()
    H, W = cam.image_height, cam.image_width
    dpix, _, _ = _maps(16, H, W)
    z = torch.zeros(1, H, W, device=DEV)
    f = fused(scene, cam, D, "invdepth", dpix, z, z)
    st = util.hip_settings(scene, cam, D, DEV)
    t = _leaves(scene)
    color, _ = GaussianRasterizer(st)(**{k: t[k] for k in NAMES})
    (color * dpix).sum().backward()
    g = _grads(t, NAMES)
    for n in NAMES:
        assert torch.equal(f[4][n], g[n]), n


def test_unused_maps_take_the_default_backward():
    """Colour-only loss through the depth_alpha rasterizer: exactly the default gradients."""
    from diff_gaussian_rasterization import GaussianRasterizer
    scene, cam, D = _c1()
    H, W = cam.image_height, cam.image_width
    dpix, _, _ = _maps(17, H, W)
    f = fused(scene, cam, D, "depth", dpix, None, None)
    t = _leaves(scene)
    color, _ = GaussianRasterizer(util.hip_settings(scene, cam, D, DEV))(**{k: t[k] for k in NAMES})
    (color * dpix).sum().backward()
    g = _grads(t, NAMES)
    for n in NAMES:
        assert torch.equal(f[4][n], g[n]), n


@pytest.mark.parametrize("mode", ["depth", "invdepth"])
def test_oracle_pin(mode):
    """D and A against the CPU oracle's blend of colors_precomp = (v, 1, 0) on a zero background."""
    scene, cam, D = gsr_scene.make_scene(3_000, -3.0, sh_degree=1, seed=21), gsr_scene.make_camera(120, 90), 1
    f = fused(scene, cam, D, mode, None, None, None, backward=False)
    v = _v(scene.means3D, cam.world_view_transform, mode)
    cols = torch.stack([v, torch.ones_like(v), torch.zeros_like(v)], 1).contiguous()
    o = util.oracle_forward(scene._replace(bg=torch.zeros(3)), cam, D, colors_precomp=cols)
    ok = o["fragile"].reshape(cam.image_height, cam.image_width) == 0
    assert ok.mean() > 0.9
    assert np.abs(f[2][0].cpu().numpy() - o["color"][0])[ok].max() <= 1e-5
    assert np.abs(f[3][0].cpu().numpy() - o["color"][1])[ok].max() <= 1e-5


@pytest.mark.parametrize("bit", ["DEBUG_NO_SPLIT", "DEBUG_TILE_SORT", "DEBUG_RADIX_DEPTH", "DEBUG_NO_TRIM"])
def test_debug_bits_and_determinism(bit):
    from diff_gaussian_rasterization import _C
    scene, cam, D = _heavy()
    H, W = cam.image_height, cam.image_width
    dpix, dD, dA = _maps(18, H, W)
    a = fused(scene, cam, D, "depth", dpix, dD, dA)
    a2 = fused(scene, cam, D, "depth", dpix, dD, dA)
    b = fused(scene, cam, D, "depth", dpix, dD, dA, debug=getattr(_C, bit))
    for x, y in ((a, a2), (a, b)):
        assert torch.equal(x[2], y[2]) and torch.equal(x[3], y[3])
    for n in NAMES:
        assert torch.equal(a[4][n], a2[4][n]), n
    if bit in ("DEBUG_NO_SPLIT", "DEBUG_TILE_SORT", "DEBUG_NO_TRIM"):
        # the backward then cuts heavy tiles into other depth segments (none, or at other list positions: the untrimmed lists are
        # longer), so accum_rec comes from other checkpoint differences -- equal to rounding, as for the colour
        # (test_boundary_gpu.py)
        for n in NAMES:
            m = float(a[4][n].abs().max())
            assert float((a[4][n] - b[4][n]).abs().max()) <= (5e-5 if n in ("scales", "rotations") else 2e-6) * max(m, 1e-30), n
    else:
        for n in NAMES:
            assert torch.equal(a[4][n], b[4][n]), n


def test_edges():
    from diff_gaussian_rasterization import GaussianRasterizer
    # P = 0
    scene, cam, D = gsr_scene.make_scene(0, -3.0, sh_degree=0, seed=1), gsr_scene.make_camera(40, 30), 0
    c, r, d, a, _ = fused(scene, cam, D, "depth", None, None, None, backward=False)
    assert d.shape == (1, 30, 40) and a.shape == (1, 30, 40) and float(d.abs().max()) == 0 and float(a.abs().max()) == 0
    # everything culled (behind the near plane)
    scene = gsr_scene.make_scene(500, -3.0, sh_degree=0, seed=2)
    scene = scene._replace(means3D=(scene.means3D * 0.01 - torch.tensor([0.0, 0.0, 20.0])).contiguous())
    c, r, d, a, _ = fused(scene, cam, D, "invdepth", None, None, None, backward=False)
    assert int(r.abs().max()) == 0 and float(d.abs().max()) == 0 and float(a.abs().max()) == 0
    # sizes that are not multiples of 16, and an image smaller than one tile
    for W, H in ((70, 45), (10, 7)):
        scene, cam, D = gsr_scene.make_scene(2_000, -3.0, sh_degree=1, seed=W), gsr_scene.make_camera(W, H), 1
        for mode in ("depth", "invdepth"):
            dpix, dD, dA = _maps(W + H, H, W)
            f = fused(scene, cam, D, mode, dpix, dD, dA)
            rr = two_pass(scene, cam, D, mode, dpix, dD, dA)
            check_forward(f, rr)
            check_grads(f[4], rr[3], two_pass(scene, cam, D, mode, dpix, dD, dA, split=True)[3], label=f"{W}x{H}/{mode}")
    # invdepth with Gaussians just beyond the 0.2 near plane (camera at z = -4 looking down +z)
    scene, cam, D = gsr_scene.make_scene(1_000, -5.0, sh_degree=0, seed=7), gsr_scene.make_camera(64, 48), 0
    g = torch.Generator().manual_seed(8)
    z = 0.2 + 0.05 * torch.rand(1_000, generator=g)
    xy = (torch.rand(1_000, 2, generator=g) - 0.5) * 0.2 * z[:, None]
    means = torch.cat([xy, (z - 4.0)[:, None]], 1)
    v = means @ cam.world_view_transform[:3, 2] + cam.world_view_transform[3, 2]
    assert float(v.min()) > 0.2 and float(v.max()) < 0.26
    scene = scene._replace(means3D=means.contiguous())
    dpix, dD, dA = _maps(9, 48, 64)
    f = fused(scene, cam, D, "invdepth", dpix, dD, dA)
    rr = two_pass(scene, cam, D, "invdepth", dpix, dD, dA)
    check_forward(f, rr)
    check_grads(f[4], rr[3], two_pass(scene, cam, D, "invdepth", dpix, dD, dA, split=True)[3], label="near")
    # unknown mode
    with pytest.raises(ValueError):
        GaussianRasterizer(util.hip_settings(scene, cam, D, DEV), depth_alpha="z")
