"""GPU parity: the HIP path (through the drop-in autograd surface -> ctypes -> C ABI) against
the CPU oracle on the same seeded inputs.

Bars: radii / tiles_touched / offsets / sorted point_list / ranges exact;
rendered RGB within 1e-5 absolute on pixels whose accept/reject decisions are not within the
oracle's margin of a threshold; n_contrib exact on those pixels; gradients within
1e-5 * max|g| (norm-wise: the reference's own atomics make them order-dependent).
"""
import numpy as np
import pytest
import torch

import grad_rows
import gsr_scene
import util

pytestmark = pytest.mark.gpu

IMG_ATOL = 1e-5
GRAD_RTOL = 1e-5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def check_forward(h, o, cam):
    P = o["P"]
    assert h["num_rendered"] == o["num_rendered"]
    np.testing.assert_array_equal(h["radii"], o["radii"])
    np.testing.assert_array_equal(h["tiles_touched"], o["tiles_touched"])
    order = np.lexsort((np.arange(P), o["depths"].view(np.uint32) | np.where(o["radii"] > 0, 0, 0xFFFFFFFF).astype(np.uint32)))
    np.testing.assert_array_equal(h["perm"], order.astype(np.uint32))
    # gradient slots: a Gaussian's first slot = exclusive prefix of tiles_touched in index order (what the reference's InclusiveSum
    # gives, rasterizer_impl.cu:323)
    assert h["slots_in_index_order"] == 1
    if h["slots_in_index_order"]:
        tt = o["tiles_touched"].astype(np.int64)
        base = np.cumsum(tt) - tt
        np.testing.assert_array_equal(h["slot_base"][tt > 0], base[tt > 0].astype(np.uint32))
    else:
        tt = o["tiles_touched"][order].astype(np.int64)
        base = np.cumsum(tt) - tt
        vis_sorted = tt > 0
        np.testing.assert_array_equal(h["slot_base"][order][vis_sorted], base[vis_sorted].astype(np.uint32))
    vis = o["radii"] > 0
    # per-Gaussian floats: bit-exact (same expression order, no FMA contraction on either side)
    for k in ("means2D", "conic_opacity", "rgb", "depths"):
        ob = o["colors_precomp"] if (k == "rgb" and o["colors_precomp"] is not None) else o[k]
        a, b = h[k][vis], ob[vis]
        assert np.array_equal(a, b), f"{k}: max abs diff {np.abs(a - b).max()}"
    cb = (o["clamped"][:, 0] | (o["clamped"][:, 1] << 1) | (o["clamped"][:, 2] << 2)).astype(np.uint8)
    np.testing.assert_array_equal(h["clamped_bits"][vis], cb[vis])
    H, W = cam.image_height, cam.image_width
    # the sorted instance list: the reference's (the oracle's), less the instances the binning was told to leave out -- tiles a splat
    # provably misses (csrc/gsr_rect_trim.h; none with GSR_DEBUG_NO_TRIM and on the tile-sort path: then the lists are the oracle's own)
    exp = util.trimmed_expectation(o, h["rshape"], W, H) if o["num_rendered"] > 0 else dict(ranges=o["ranges"], n_contrib=o["n_contrib"])
    if o["num_rendered"] > 0:
        np.testing.assert_array_equal(h["point_list"], exp["point_list"])
        np.testing.assert_array_equal(h["keys"], exp["keys"])
    np.testing.assert_array_equal(h["ranges"], exp["ranges"])
    ok = o["fragile"] == 0
    frac = 1.0 - ok.mean()
    assert frac < 5e-3, f"too many fragile pixels: {frac}"
    np.testing.assert_array_equal(h["n_contrib"][ok], exp["n_contrib"][ok])
    err = np.abs(h["color"].reshape(3, -1) - o["color"].reshape(3, -1))[:, ok]
    assert err.max() <= IMG_ATOL, f"image max abs err {err.max()} (mean {err.mean()})"
    errT = np.abs(h["final_T"] - o["final_T"])[ok]
    assert errT.max() <= IMG_ATOL
    return err.max()


def _nerr(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / max(np.abs(b).max(), 1e-20))


def check_rows(h, o, dpix, label=None):
    """The per-row level of check_grads: every row and component of the HIP blend sums (dL_dmeans2D, dL_dconic, dL_dopacity,
    dL_dcolors of raw_grads) within the row's own float64 bound, |hip - S| <= E = 2^-24 (B + n A) of
    oracle.blend_backward_budget (derived in tests/test_grad_rows_gpu.py), and +0 bits in every row without terms."""
    # the depth segments of a heavy tile start every GSR_CKPT_STRIDE-th position of the list the binning kept
    kept = util.trimmed_expectation(o, h["rshape"], o["W"], o["H"])["kept"] if o["num_rendered"] > 0 else None
    bud = util.oracle.blend_backward_budget(o, dpix.numpy(), restart_at=util.oracle.restart_positions(o, kept) if o["num_rendered"] > 0 else None)
    ratios, bad = grad_rows.rows_failures(h["raw_grads"], bud)
    msg = grad_rows.format_ratios(ratios)
    print(msg)
    util.parity_log(f"[{label or 'case'}] blend sums per row: largest |hip - float64| / E\n" + msg)
    assert not bad, "a row of the blend sums lies outside its float64 bound:\n" + "\n".join(bad) + "\n" + msg
    return ratios


def check_grads(h, o, dpix, names, label=None, og=None, rows=True):
    """Four levels.
    (0) per row (check_rows above): every Gaussian's row of the blend sums within its own float64 bound -- the three levels below
        speak for the few rows with the largest gradients only.  rows=False leaves the level out; a caller says why.
    (1) backward blend kernel alone: its per-Gaussian sums (dL_dmean2D, dL_dconic, dL_dopacity,
        dL_dcolors) against the oracle's double-precision sums, 1e-5 norm-wise.
    (2) per-Gaussian chain alone: the HIP outputs against the oracle's chain evaluated on the HIP
        kernel's OWN blend sums (identical inputs, same fp32 expression order): 1e-6.
    (3) end to end through autograd: 1e-5 norm-wise, or the reference's own reproducibility band
        where that is larger: its backward sums with fp32 atomics in hardware order, so two runs
        of the reference differ; the oracle measures that spread by accumulating in fp32 in two
        different tile orders (accum_mode 1 / 2) and the bar is max(1e-5, 2 x spread)."""
    if rows:
        check_rows(h, o, dpix, label)
    if og is None:
        og = util.oracle.backward(o, dpix.numpy())
    raw = h["raw_grads"]
    P = o["P"]
    report = []
    g1 = util.oracle.backward(o, dpix.numpy(), accum_mode=1)
    g2 = util.oracle.backward(o, dpix.numpy(), accum_mode=2)

    def bar(k):
        band = max(_nerr(g1[k], og[k]), _nerr(g2[k], og[k]), _nerr(g1[k], g2[k]))
        return max(GRAD_RTOL, 2.0 * band)

    for k in ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors"):
        e = _nerr(raw[k].reshape(P, -1), og[k].reshape(P, -1))
        report.append((f"blend:{k}", e, bar(k)))
    oc = util.oracle.gaussian_backward(o, raw["dL_dmeans2D"], raw["dL_dconic"], raw["dL_dcolors"])
    for k in ("dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations"):
        if raw[k].size:
            report.append((f"chain:{k}", _nerr(raw[k].reshape(P, -1), oc[k].reshape(P, -1)), 1e-6))
    for k in names:
        report.append((f"e2e:{k}", _nerr(h["grads"][k], og[k]), bar(k)))
    bad = [r for r in report if not (r[1] <= r[2])]
    msg = "\n".join(f"{n:28s} err {e:.3e}  bar {b:.3e}" for n, e, b in report)
    print(msg)
    util.parity_log(f"[{label or 'case'}] gradient error vs bar (max-abs / max|g|)\n" + msg)
    assert not bad, "gradient parity failed:\n" + msg
    return report


CASES = [
    # name, P, W, H, D, mu, seed
    ("c1_like", 10_000, 256, 256, 0, -3.5, 0),
    ("partial_tiles_deg3", 3_000, 200, 120, 3, -3.0, 3),
    ("deg1", 2_000, 97, 61, 1, -2.5, 5),
    ("deg2_big_splats", 500, 160, 96, 2, -1.5, 6),
]


@pytest.mark.parametrize("name,P,W,H,D,mu,seed", CASES)
def test_forward_backward_vs_oracle(name, P, W, H, D, mu, seed):
    _need_gpu()
    scene = gsr_scene.make_scene(P, mu, sh_degree=D, seed=seed)
    cam = gsr_scene.make_camera(W, H)
    o = util.oracle_forward(scene, cam, D)
    dpix = util.fragile_free_dpix(o, cam)
    h = util.hip_forward_backward(scene, cam, D, dpix)
    err = check_forward(h, o, cam)
    util.parity_log(f"[{name}] P={P} {W}x{H} deg {D}: R={o['num_rendered']}, integer state exact, image max-abs (non-fragile) {err:.3e}")
    check_grads(h, o, dpix, ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"], label=name)


def test_rotated_camera_and_sh_degree_below_max():
    """16 coefficients stored but active degree 1 (training's early phase): unused dL_dsh rows are 0."""
    _need_gpu()
    scene = gsr_scene.make_scene(4_000, -3.0, sh_degree=3, seed=11)
    cam = gsr_scene.ring_camera(320, 180, k=3, n=8)
    o = util.oracle_forward(scene, cam, 1)
    dpix = util.fragile_free_dpix(o, cam)
    h = util.hip_forward_backward(scene, cam, 1, dpix)
    check_forward(h, o, cam)
    check_grads(h, o, dpix, ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"])
    assert np.all(h["grads"]["dL_dsh"][:, 4:, :] == 0)


def test_precomputed_colors_and_cov3d_and_scale_modifier():
    _need_gpu()
    scene = gsr_scene.make_scene(2_500, -3.0, sh_degree=0, seed=21)
    cam = gsr_scene.make_camera(180, 100)
    g = torch.Generator().manual_seed(5)
    colors = torch.rand(2_500, 3, generator=g)
    # covariances from the oracle's own computeCov3D at scale_modifier 1.3
    o0 = util.oracle_forward(scene, cam, 0, scale_modifier=1.3)
    cov = torch.from_numpy(o0["cov3D"].copy())
    vis = o0["radii"] > 0
    cov[~torch.from_numpy(vis)] = torch.eye(3)[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]] * 1e-4
    o = util.oracle_forward(scene, cam, 0, colors_precomp=colors, cov3D_precomp=cov, use_sh=False, use_scale_rot=False)
    dpix = util.fragile_free_dpix(o, cam)
    h = util.hip_forward_backward(scene, cam, 0, dpix, colors_precomp=colors, cov3D_precomp=cov, use_sh=False,
                                  use_scale_rot=False)
    check_forward(h, o, cam)
    check_grads(h, o, dpix, ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dcolors", "dL_dcov3D"])
    # scale_modifier path with scales/rotations
    o2 = util.oracle_forward(scene, cam, 0, scale_modifier=1.3)
    dpix2 = util.fragile_free_dpix(o2, cam)
    h2 = util.hip_forward_backward(scene, cam, 0, dpix2, scale_modifier=1.3)
    check_forward(h2, o2, cam)
    check_grads(h2, o2, dpix2, ["dL_dmeans3D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"])


def test_edge_cases_empty_scene_and_nothing_visible():
    _need_gpu()
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    cam = gsr_scene.make_camera(64, 48)
    scene = gsr_scene.make_scene(10, -3.0, sh_degree=0, seed=1)
    settings = util.hip_settings(scene, cam, 0, dev)
    # P == 0: image stays zero-filled, not background (rasterize_points.cu:94,129)
    e3 = torch.zeros(0, 3, device=dev)
    color, radii = GaussianRasterizer(settings)(means3D=e3, means2D=e3.clone(), opacities=torch.zeros(0, 1, device=dev),
                                                shs=torch.zeros(0, 1, 3, device=dev), scales=e3.clone(),
                                                rotations=torch.zeros(0, 4, device=dev))
    assert color.shape == (3, 48, 64) and radii.shape == (0,)
    assert float(color.abs().max()) == 0.0
    # everything behind the camera: R == 0, every pixel is background (T = 1), grads are zero
    behind = gsr_scene.Scene(scene.means3D - torch.tensor([0.0, 0.0, 100.0]), scene.scales, scene.rotations,
                             scene.opacities, scene.shs, scene.bg)
    dpix = torch.ones(3, 48, 64)
    h = util.hip_forward_backward(behind, cam, 0, dpix)
    assert h["num_rendered"] == 0 and np.all(h["radii"] == 0)
    np.testing.assert_array_equal(h["color"], np.broadcast_to(scene.bg.numpy()[:, None, None], (3, 48, 64)))
    for k, v in h["grads"].items():
        assert np.all(v == 0), k


def test_mark_visible():
    _need_gpu()
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    scene = gsr_scene.make_scene(5000, -3.0, sh_degree=0, seed=2)
    cam = gsr_scene.ring_camera(64, 64, 1, 8, radius=1.0)
    vis = GaussianRasterizer(util.hip_settings(scene, cam, 0, dev)).markVisible(scene.means3D.to(dev))
    ref = util.oracle.mark_visible(scene.means3D.numpy(), cam.world_view_transform.numpy(), cam.full_proj_transform.numpy())
    assert vis.dtype == torch.bool
    np.testing.assert_array_equal(vis.cpu().numpy(), ref)
    assert 0 < ref.sum() < 5000


def test_validation_errors_match_reference_text():
    _need_gpu()
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    scene = gsr_scene.make_scene(10, -3.0, sh_degree=0, seed=1)
    cam = gsr_scene.make_camera(32, 32)
    r = GaussianRasterizer(util.hip_settings(scene, cam, 0, dev))
    m = scene.means3D.to(dev)
    with pytest.raises(Exception, match="Please provide excatly one of either SHs or precomputed colors!"):
        r(means3D=m, means2D=m, opacities=scene.opacities.to(dev), scales=scene.scales.to(dev), rotations=scene.rotations.to(dev))
    with pytest.raises(Exception, match="Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"):
        r(means3D=m, means2D=m, opacities=scene.opacities.to(dev), shs=scene.shs.to(dev), scales=scene.scales.to(dev))
    # no CPU fallback: CPU tensors are refused loudly
    with pytest.raises(RuntimeError, match="no CPU path"):
        r(means3D=scene.means3D, means2D=scene.means3D, opacities=scene.opacities, shs=scene.shs, scales=scene.scales,
          rotations=scene.rotations)


def test_prefiltered_flag_reports_instead_of_trapping():
    _need_gpu()
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    scene = gsr_scene.make_scene(100, -3.0, sh_degree=0, seed=1)
    cam = gsr_scene.ring_camera(32, 32, 1, 8, radius=1.0)  # some points behind the camera
    r = GaussianRasterizer(util.hip_settings(scene, cam, 0, dev, prefiltered=True))
    m = scene.means3D.to(dev)
    with pytest.raises(RuntimeError, match="filtered although prefiltered"):
        r(means3D=m, means2D=m, opacities=scene.opacities.to(dev), shs=scene.shs.to(dev), scales=scene.scales.to(dev),
          rotations=scene.rotations.to(dev))


def test_hip_sh_colour_and_gradient_match_reference_fixture_directly():
    """The HIP per-Gaussian kernels against sh_golden.npz (the reference's own eval_sh and its autograd), not through
    the oracle: preprocess's rgb and clamp bits (forward.cu:21-81), gaussian_backward's dL_dsh and the view-direction
    part of dL_dmean3D (backward.cu:20-139).  The fixture's points are rendered as isotropic splats by a camera at the
    fixture's camera position; the blend sums are dictated through dL_dcolors of a precomputed-colour twin run."""
    _need_gpu()
    import os
    from diff_gaussian_rasterization import _C
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sh_golden.npz"))
    dev = torch.device("cuda:0")
    pos, campos, shs = torch.from_numpy(g["pos"]), torch.from_numpy(g["campos"]), torch.from_numpy(g["shs"])
    n = pos.shape[0]
    cam = gsr_scene.make_camera(256, 256, fovx=1.2, R=np.eye(3), T=-campos.numpy().astype(np.float64))
    np.testing.assert_allclose(cam.camera_center.numpy(), campos.numpy(), atol=1e-6)
    scene = gsr_scene.Scene(pos.contiguous(), torch.full((n, 3), 0.02), torch.tensor([[1.0, 0, 0, 0]]).repeat(n, 1), torch.full((n, 1), 0.7),
                            shs.contiguous(), torch.zeros(3))
    dpix = torch.randn(3, 256, 256, generator=torch.Generator().manual_seed(5))
    for deg in range(4):
        st = util.hip_settings(scene, cam, deg, dev)
        # campos is handed to the kernels exactly as the fixture has it (the camera's own differs in the last bit)
        st = st._replace(campos=campos.to(dev))
        e = torch.empty(0, device=dev)
        t = {k: getattr(scene, k).to(dev) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
        R, color, radii, geom, binning, img = _C.rasterize_gaussians(
            st.bg, t["means3D"], e, t["opacities"], t["scales"], t["rotations"], 1.0, e, st.viewmatrix, st.projmatrix, st.tanfovx,
            st.tanfovy, 256, 256, t["shs"], deg, st.campos, False, False)
        vis = (radii > 0).cpu().numpy()
        assert vis.sum() > 0.8 * n
        state = util.unpack_state(dict(R=R, geom=geom, binning=binning, img=img), n, 256, 256)
        np.testing.assert_allclose(state["rgb"][vis], g[f"rgb_deg{deg}"][vis], rtol=0, atol=2e-6)
        raw = g[f"raw_deg{deg}"]
        sure = vis[:, None] & (np.abs(raw) > 1e-5)
        bits = np.stack([(state["clamped_bits"] >> c) & 1 for c in range(3)], 1).astype(bool)
        assert np.array_equal(bits[sure], (raw < 0)[sure]) and bits[vis].any()
        grads = _C.rasterize_gaussians_backward(st.bg, t["means3D"], radii, e, t["scales"], t["rotations"], 1.0, e, st.viewmatrix, st.projmatrix,
                                                st.tanfovx, st.tanfovy, dpix.to(dev), t["shs"], deg, st.campos, geom, R, binning, img, False)
        dL_dmeans2D, dL_dcolors, _, dL_dmeans3D, _, dL_dsh, _, _ = grads
        # the reference fixture holds d(sum(colors * dL_dcolor))/d(sh, pos) for ITS dL_dcolor; the kernel's SH backward is
        # linear in dL_dcolor, so feed the kernel's own blend sums to autograd of the reference formula: eval_sh is not
        # importable on the GPU box, but dL_dsh = basis x (clamp-masked dL_dcolor) lets the fixture's gradient be rescaled
        # per Gaussian and channel wherever its own dL_dcolor is not ~0
        dcol = dL_dcolors.cpu().numpy()
        fix_dcol = g["dL_dcolor"]
        used = (deg + 1) ** 2
        ok = vis[:, None] & (np.abs(fix_dcol) > 1e-2)
        ratio = np.where(ok, dcol / np.where(ok, fix_dcol, 1.0), 0.0)                       # (n,3)
        want_dsh = g[f"dL_dsh_deg{deg}"] * ratio[:, None, :]
        got_dsh = dL_dsh.cpu().numpy()
        sel = np.broadcast_to(ok[:, None, :], got_dsh.shape)
        scale = max(np.abs(want_dsh[sel]).max(), 1e-30)
        assert np.abs(got_dsh - want_dsh)[sel].max() <= 1e-5 * scale
        assert np.all(got_dsh[:, used:, :] == 0)


def test_depth_sort_pass_count_follows_depth_range():
    """The depth order of the Gaussians, both ways it is produced.  Up to 2 Mi Gaussians: top-digit buckets sorted inside LDS
    (csrc/depthsort.hip), three launches whatever the depth range, result in (depth_keys, perm).  GSR_DEBUG_RADIX_DEPTH (and
    longer lists): global radix passes on (depth bits - smallest depth bits), only those the bits need -- three when the view's
    depth range spans fewer than 2^24 float steps (result in the ping-pong partner arrays), four otherwise.  Every variant must
    give the oracle's order exactly (ties, culled Gaussians last)."""
    _need_gpu()
    from diff_gaussian_rasterization import _C
    # (a) compact depth range: camera at distance 4 from a cube of side 3 -> depths 2.5 .. 5.5
    scene = gsr_scene.make_scene(6000, -3.0, sh_degree=1, seed=13)
    cam = gsr_scene.make_camera(160, 96)
    o = util.oracle_forward(scene, cam, 1)
    h = util.hip_forward_backward(scene, cam, 1, None)
    check_forward(h, o, cam)
    assert h["depth_sort_result_in_alt"] == 0
    h = util.hip_forward_backward(scene, cam, 1, None, debug=_C.DEBUG_RADIX_DEPTH)
    check_forward(h, o, cam)
    assert h["depth_sort_result_in_alt"] == 1
    # (b) depths from 0.2 to ~200: the float bits span more than 2^24 steps
    g = torch.Generator().manual_seed(3)
    means = scene.means3D.clone()
    means[:, 2] = torch.exp(torch.rand(6000, generator=g) * 7.0 - 1.7) - 4.0   # view-space z = means.z + 4 in (0.18, 200)
    means[:, :2] *= (means[:, 2:3] + 4.0) * 0.3
    means[::50] = means[7]                                                        # clones: equal depth keys
    far = scene._replace(means3D=means.contiguous(), scales=(scene.scales * (means[:, 2:3] + 4.0).clamp(min=0.3)).contiguous())
    o = util.oracle_forward(far, cam, 1)
    z = o["depths"][o["radii"] > 0]
    assert z.min() < 0.5 and z.max() > 100.0
    for dbg in (False, _C.DEBUG_RADIX_DEPTH):
        h = util.hip_forward_backward(far, cam, 1, None, debug=dbg)
        check_forward(h, o, cam)
        assert h["depth_sort_result_in_alt"] == 0


def test_smoke_entry():
    _need_gpu()
    import __graft_entry__
    __graft_entry__.smoke()


def test_hip_against_the_independent_pytorch_splat():
    """A second derivation that shares no code with the C oracle: oracle/torch_tile_splat.py restates the forward in
    vectorised PyTorch ops with its OWN projection, binning and sort, and leaves the gradients to torch.autograd.  The HIP
    path must give the same instance count and radii, the same image (fp32 vs fp32, non-fragile pixels) and gradients that
    agree with autograd to the fp32 noise of a 200x120 render (the oracle only lends its fragile-pixel flags)."""
    _need_gpu()
    from oracle import torch_tile_splat
    scene = gsr_scene.make_scene(3000, -3.0, sh_degree=3, seed=23)
    cam = gsr_scene.ring_camera(200, 120, 1, 8, radius=3.0)
    o = util.oracle_forward(scene, cam, 3, margin=1e-3)
    dpix = util.fragile_free_dpix(o, cam, seed=9)
    h = util.hip_forward_backward(scene, cam, 3, dpix)
    leaves = [t.clone().requires_grad_(True) for t in (scene.means3D, scene.scales, scene.rotations, scene.opacities, scene.shs)]
    img, radii, R = torch_tile_splat.render(*leaves, cam.world_view_transform, cam.full_proj_transform, cam.camera_center, scene.bg,
                                            cam.image_width, cam.image_height, cam.tanfovx, cam.tanfovy, 3)
    assert R == h["num_rendered"]
    np.testing.assert_array_equal(radii.numpy(), h["radii"])
    ok = (o["fragile"] == 0).reshape(cam.image_height, cam.image_width)
    err = np.abs(img.detach().numpy() - h["color"])[:, ok].max()
    assert err < 2e-5, err
    (img * dpix).sum().backward()
    names = ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacity", "dL_dsh")
    for k, leaf in zip(names, leaves):
        a, b = h["grads"][k].reshape(3000, -1), leaf.grad.numpy().reshape(3000, -1)
        e = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-20))
        print(k, e)
        assert e < 1e-4, (k, e)   # both sides fp32, sums in different orders (measured 1e-6 ... 1.5e-5)
