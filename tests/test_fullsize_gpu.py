"""GPU, BASELINE.json's full sizes.  C2 (100k Gaussians, SH deg 3, 1980x1080): complete parity with the
oracle.  C3 (1M, the headline workload) and C5 (6M Gaussians at 4K): size-independent properties --
sorted instance list, ranges that partition it, bitwise run-to-run determinism (the reference's
atomics cannot offer it), exact linearity of the backward in the upstream gradient."""
import numpy as np
import pytest
import torch

import gsr_scene
import util
from test_parity_gpu import check_forward, check_grads

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


NAMES = ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"]


def _bars(o, dpix_np, og, names):
    """max(1e-5, 2 x the reference's own reproducibility band) per tensor: fp32 accumulation in two tile orders."""
    g1 = util.oracle.backward(o, dpix_np, accum_mode=1)
    g2 = util.oracle.backward(o, dpix_np, accum_mode=2)
    n = lambda a, b: float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / max(np.abs(b).max(), 1e-20))
    return {k: max(1e-5, 2.0 * max(n(g1[k], og[k]), n(g2[k], og[k]), n(g1[k], g2[k]))) for k in names}


def exclusion_figures(name, scene, cam, D, o, h):
    """What the parity bars leave out, printed next to them: the fragile-pixel fraction, the image error over ALL pixels
    (fragile ones included), and the gradient error when the upstream gradient is NOT zeroed on the fragile pixels.
    A fragile pixel is one where a 1-ulp difference of exp() legitimately flips alpha < 1/255 or T(1-alpha) < 1e-4; the
    pixel then moves by up to alpha*T (~4e-3), which is why these are reported, and bounded loosely, not held to 1e-5.

    Then the attribution, as a test: the pixels where the two images actually differ by more than 1e-5 ARE the flipped
    decisions (a handful per million), and with the upstream gradient zeroed on exactly those pixels -- nothing else
    masked, no oracle-side margin involved -- every gradient tensor is inside its bar again."""
    ok = o["fragile"] == 0
    diff = np.abs(h["color"].reshape(3, -1) - o["color"].reshape(3, -1))
    frag = float(1.0 - ok.mean())
    full_max, ok_max = float(diff.max()), float(diff[:, ok].max())
    g = torch.Generator().manual_seed(1)
    dpix = torch.randn(3, cam.image_height, cam.image_width, generator=g)   # unmasked
    hu = util.hip_forward_backward(scene, cam, D, dpix)
    og = util.oracle.backward(o, dpix.numpy())
    rel = {k: float(np.abs(hu["grads"][k].astype(np.float64) - og[k]).max() / max(np.abs(og[k]).max(), 1e-30)) for k in NAMES}
    line = (f"[{name}] fragile pixels {frag:.3e} of the image; image max-abs error: all pixels {full_max:.3e}, non-fragile {ok_max:.3e}; "
            "gradient error with UNMASKED dL/dpix (max-abs / max|g|): " + ", ".join(f"{k} {v:.2e}" for k, v in rel.items()))
    print(line)
    util.parity_log(line)
    assert frag < 5e-3 and full_max < 2e-2 and max(rel.values()) < 2e-3
    # flip attribution
    flipped = diff.max(axis=0) > 1e-5
    assert not (flipped & ok).any(), "every observed difference lies on a pixel the oracle flagged as fragile"
    nflip = int(flipped.sum())
    keep = torch.from_numpy(~flipped).reshape(cam.image_height, cam.image_width)
    dpix2 = dpix * keep
    h2 = util.hip_forward_backward(scene, cam, D, dpix2)
    og2 = util.oracle.backward(o, dpix2.numpy())
    bars = _bars(o, dpix2.numpy(), og2, NAMES)
    rel2 = {k: float(np.abs(h2["grads"][k].astype(np.float64) - og2[k]).max() / max(np.abs(og2[k]).max(), 1e-30)) for k in NAMES}
    line = (f"[{name}] flip attribution: {nflip} of {flipped.size} pixels differ by more than 1e-5 (all of them flagged fragile; "
            f"{int((~ok).sum())} flagged in total); with dL/dpix zeroed on those {nflip} pixels only: " +
            ", ".join(f"{k} {rel2[k]:.2e} (bar {bars[k]:.2e})" for k in NAMES))
    print(line)
    util.parity_log(line)
    bad = [k for k in NAMES if not rel2[k] <= bars[k]]
    assert not bad, f"gradients outside their bars after removing the flipped pixels: {bad}\n{line}"
    return frag, full_max, rel


def _full_parity(name, rows=True):
    scene, cam, D = gsr_scene.make_config(name)
    o = util.oracle_forward(scene, cam, D)
    dpix = util.fragile_free_dpix(o, cam)
    from diff_gaussian_rasterization import _C
    h = util.hip_forward_backward(scene, cam, D, dpix)
    err = check_forward(h, o, cam)
    # ... and with every tile of every rectangle binned (GSR_DEBUG_NO_TRIM): the reference's own lists, and the same image bit for bit
    h0 = util.hip_forward_backward(scene, cam, D, None, debug=_C.DEBUG_NO_TRIM)
    check_forward(h0, o, cam)
    assert len(h0["point_list"]) == o["num_rendered"] and np.array_equal(h0["color"], h["color"]) and np.array_equal(h0["final_T"], h["final_T"])
    util.parity_log(f"[{name}] P={o['P']} {cam.image_width}x{cam.image_height} deg {D}: R={o['num_rendered']}, radii / tiles / "
                    f"point_list / keys / ranges / n_contrib exact (binning every tile: the oracle's lists; default: the oracle's lists less the "
                    f"{o['num_rendered'] - len(h['point_list'])} instances the trim words name, {len(h['point_list'])} listed), image identical in both, "
                    f"max-abs (non-fragile) {err:.3e}")
    check_grads(h, o, dpix, NAMES, label=name, rows=rows)
    return scene, cam, D, o, h


def test_c2_full_parity_with_oracle():
    _need_gpu()
    exclusion_figures("C2", *_full_parity("C2"))


def test_c3_full_parity_with_oracle():
    """The headline workload (1M Gaussians, 1980x1080, SH degree 3) against the oracle in full: every integer output
    exact, image and gradients to the same bars as the small cases; then the flip attribution of exclusion_figures."""
    _need_gpu()
    # rows=False: the float64 walk of the per-row level takes some ten CPU seconds at this size; C2 above keeps the level at full resolution
    exclusion_figures("C3", *_full_parity("C3", rows=False))


def test_c5_full_parity_with_oracle():
    """6M Gaussians at 3840x2160 (R = 7.1e7): radii, tiles, sorted instance list, 64-bit keys, tile ranges exact; image
    1e-5 and n_contrib exact on the non-fragile pixels; and every gradient against the oracle's backward
    (backward.cu:408-601 at this size), same bars as everywhere."""
    _need_gpu()
    _full_parity("C5", rows=False)   # the per-row level's float64 walk over 7.1e7 instances: tens of CPU seconds


def test_c4_eight_views_summed_gradients_match_oracle(tmp_path):
    """BASELINE.json configs[3] on one GPU: the 8 ring cameras of the view-parallel bench (bench.py, ring_camera(k, 8)) at
    the 1M-Gaussian scene, rendered one after the other.  Per view: every integer output exact and the image to 1e-5
    against the oracle.  Over the views: the sum of the parameter gradients -- what the 8-rank step hands to the
    optimiser -- from (a) the plain rasterizer, (b) rasterize_view_parallel with the 'compact' and (c) the 'allreduce'
    exchange (world 1: the collectives are no-ops, everything else of the N > 1 backward runs) against the sum of the
    eight oracle backwards, bars = max(1e-5, 2 x the band of the SUMMED fp32-accumulated oracle gradients)."""
    _need_gpu()
    import view_parallel
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    P, W, H, D, mu = gsr_scene.CONFIGS["C3"]
    scene = gsr_scene.make_scene(P, mu, D, seed=0)
    keys = dict(means3D="dL_dmeans3D", shs="dL_dsh", opacities="dL_dopacity", scales="dL_dscales", rotations="dL_drotations")
    leaves = {k: getattr(scene, k).to(dev) for k in keys}
    ex = {m: view_parallel.GradientExchange(P, 16, dev, sh_mode=m, parts=2) for m in ("compact", "allreduce")}
    total = {m: {k: torch.zeros_like(v) for k, v in leaves.items()} for m in ("plain", "compact", "allreduce")}
    want = {n: 0.0 for n in keys.values()}
    band = {1: {n: 0.0 for n in keys.values()}, 2: {n: 0.0 for n in keys.values()}}
    stats = []
    for v in range(8):
        cam = gsr_scene.ring_camera(W, H, k=v, n=8)
        o = util.oracle_forward(scene, cam, D)
        dpix = util.fragile_free_dpix(o, cam, seed=1 + v)
        h = util.hip_forward_backward(scene, cam, D, None)
        err = check_forward(h, o, cam)
        stats.append(dict(view=v, V=int((o["radii"] > 0).sum()), R=int(o["num_rendered"]), image_maxabs=float(err)))
        dnp = dpix.numpy()
        og = util.oracle.backward(o, dnp)
        g1, g2 = util.oracle.backward(o, dnp, accum_mode=1), util.oracle.backward(o, dnp, accum_mode=2)
        for n in keys.values():
            want[n] = want[n] + og[n].astype(np.float64)
            band[1][n] = band[1][n] + g1[n].astype(np.float64)
            band[2][n] = band[2][n] + g2[n].astype(np.float64)
        del o, og, g1, g2
        st = util.hip_settings(scene, cam, D, dev)
        dd = dpix.to(dev)
        for mode in total:
            p = {k: t.clone().requires_grad_(True) for k, t in leaves.items()}
            m2 = torch.zeros_like(p["means3D"], requires_grad=True)
            if mode == "plain":
                color, _ = GaussianRasterizer(st)(means2D=m2, **p)
            else:
                color, _ = view_parallel.rasterize_view_parallel(p["means3D"], m2, p["shs"], p["opacities"], p["scales"], p["rotations"], st, ex[mode])
            color.backward(dd)
            for k in keys:
                total[mode][k] += p[k].grad
        torch.cuda.synchronize()
    n = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-20))
    bars = {k: max(1e-5, 2.0 * max(n(band[1][k], want[k]), n(band[2][k], want[k]), n(band[1][k], band[2][k]))) for k in want}
    lines = ["[C4] 8 ring views of the C3 scene, per view: " + "; ".join(f"v{s['view']} V={s['V']} R={s['R']} img {s['image_maxabs']:.1e}" for s in stats)]
    bad = []
    for mode in total:
        errs = {keys[k]: n(total[mode][k].cpu().numpy().astype(np.float64), want[keys[k]]) for k in keys}
        lines.append(f"[C4] summed gradients over 8 views, {mode}: " + ", ".join(f"{k} {e:.2e} (bar {bars[k]:.2e})" for k, e in errs.items()))
        bad += [(mode, k) for k, e in errs.items() if not e <= bars[k]]
    # the two exchange modes and the plain rasterizer add the same per-view gradients: world-1 results are bit-identical
    for k in keys:   # ('compact' rebuilds dL_dsh as basis x dL/dRGB with its own kernel: the same products, the same bits)
        assert torch.equal(total["plain"][k], total["allreduce"][k]) and torch.equal(total["plain"][k], total["compact"][k]), k
    for l in lines:
        print(l)
        util.parity_log(l)
    assert not bad, "\n".join(lines)


def _list_structure(cap, radii, P, W, H, T, dev, whole):
    """Size-independent properties of the sorted instance list of one forward: sorted by tile, by depth inside a tile, ties in index
    order; every instance inside its Gaussian's rectangle, no (tile, Gaussian) pair twice; the ranges partition the list.  whole:
    the run binned every tile of every rectangle (GSR_DEBUG_NO_TRIM) -- then every rectangle tile appears exactly once and the list
    has num_rendered entries; otherwise at most once, and fewer.  Returns the number of listed instances."""
    from diff_gaussian_rasterization import _C
    R = cap["R"]
    gl, il, bl = _C.geometry_layout(P), _C.image_layout(W, H), _C.binning_layout(P, R, W, H)
    u32 = lambda buf, off, n: buf[off:off + 4 * n].view(torch.int32)
    tiles_touched = u32(cap["geom"], gl.tiles_touched, P).to(torch.int64)
    assert int(tiles_touched.sum()) == R
    assert torch.equal(tiles_touched > 0, radii > 0)
    ranges = u32(cap["img"], il.ranges, 2 * T).view(T, 2).to(torch.int64)
    lens = ranges[:, 1] - ranges[:, 0]
    L = int(lens.sum())
    assert (L == R if whole else L <= R) and bool((lens >= 0).all())
    if int(bl.column_pairs):
        # column-pair binning: no per-instance keys are stored; the tile of instance i is the tile whose range holds i.  The
        # ranges must partition [0, R) in tile order ...
        ne0 = lens > 0
        assert torch.equal(ranges[ne0, 0], torch.cumsum(lens[ne0], 0) - lens[ne0])
        tile_keys = torch.repeat_interleave(torch.arange(T, device=dev), lens)
    else:
        kb = int(bl.tile_key_bytes)
        tile_keys = cap["binning"][bl.tile_keys:bl.tile_keys + kb * L].view(torch.int16 if kb == 2 else torch.int32).to(torch.int64) & (0xFFFF if kb == 2 else 0xFFFFFFFF)
    plist = u32(cap["binning"], bl.point_list, L).to(torch.int64)
    assert bool((tile_keys[1:] >= tile_keys[:-1]).all()), "instances sorted by tile"
    assert int(tile_keys.max()) < T
    # depth bits per Gaussian from the depth sort's outputs
    in_alt = int(u32(cap["geom"], gl.status, 4)[2])   # the depth sort's result: in the ping-pong partners after three passes
    perm = u32(cap["geom"], gl.perm_alt if in_alt else gl.perm, P).to(torch.int64)
    skeys = u32(cap["geom"], gl.depth_keys_alt if in_alt else gl.depth_keys, P).to(torch.int64) & 0xFFFFFFFF
    assert bool((skeys[1:] >= skeys[:-1]).all()), "Gaussians sorted by depth"
    assert torch.equal(torch.sort(perm).values, torch.arange(P, device=dev)), "perm is a permutation"
    depth_of = torch.empty(P, dtype=torch.int64, device=dev)
    depth_of[perm] = skeys
    d = depth_of[plist]
    same_tile = tile_keys[1:] == tile_keys[:-1]
    assert bool((d[1:][same_tile] >= d[:-1][same_tile]).all()), "depth-sorted inside every tile"
    tie = same_tile & (d[1:] == d[:-1])
    assert bool((plist[1:][tie] > plist[:-1][tie]).all()), "stable: equal keys keep ascending Gaussian index"
    # ... and every instance must sit in a tile of its Gaussian's rectangle, every rectangle tile exactly once: per tile, the
    # number of instances = the number of rectangles that cover it (a 2-D difference array over the tile grid)
    gxt = (W + 15) // 16
    rect = u32(cap["geom"], gl.rect, 2 * P).view(P, 2).to(torch.int64)
    rx0, ry0, rw, rh = rect[:, 0] & 0xFFFF, rect[:, 0] >> 16, rect[:, 1] & 0xFFFF, (rect[:, 1] >> 16) & 0xFFFF
    tx, ty = tile_keys % gxt, tile_keys // gxt
    gi = plist
    assert bool(((tx >= rx0[gi]) & (tx < rx0[gi] + rw[gi]) & (ty >= ry0[gi]) & (ty < ry0[gi] + rh[gi])).all()), "instance outside its Gaussian's rectangle"
    gyt = (H + 15) // 16
    diff = torch.zeros((gyt + 1) * (gxt + 1), dtype=torch.int64, device=dev)
    vis = (rw * rh) > 0
    for sx, sy, sign in ((rx0, ry0, 1), (rx0 + rw, ry0, -1), (rx0, ry0 + rh, -1), (rx0 + rw, ry0 + rh, 1)):
        diff.index_add_(0, (sy[vis] * (gxt + 1) + sx[vis]), torch.full((int(vis.sum()),), sign, dtype=torch.int64, device=dev))
    cover = diff.view(gyt + 1, gxt + 1).cumsum(0).cumsum(1)[:gyt, :gxt].reshape(-1)
    assert torch.equal(cover, lens) if whole else bool((lens <= cover).all()), "per-tile instance counts differ from the rectangles' coverage"
    key2 = tile_keys * P + plist
    assert int(torch.unique(key2).numel()) == L, "a (tile, Gaussian) pair appears twice"
    counts = torch.bincount(tile_keys, minlength=T)
    assert torch.equal(counts, lens)
    ne = lens > 0
    assert torch.equal(tile_keys[ranges[ne, 0]], torch.nonzero(ne).flatten())
    return L


def _properties(name, check_linearity=True):
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    dev = torch.device("cuda:0")
    scene, cam, D = gsr_scene.make_config(name)
    P, W, H = scene.means3D.shape[0], cam.image_width, cam.image_height
    T = ((W + 15) // 16) * ((H + 15) // 16)
    settings = util.hip_settings(scene, cam, D, dev)
    leaves = dict(means3D=scene.means3D, shs=scene.shs, opacities=scene.opacities, scales=scene.scales,
                  rotations=scene.rotations)
    g = torch.Generator().manual_seed(2)
    dpix = torch.randn(3, H, W, generator=g).to(dev)

    def run(scale, debug=0):
        p = {k: v.to(dev).clone().requires_grad_(True) for k, v in leaves.items()}
        means2D = torch.zeros_like(p["means3D"], requires_grad=True)
        cap = {}
        orig = _C.rasterize_gaussians

        def spy(*a):
            r = orig(*a)
            cap["R"], cap["geom"], cap["binning"], cap["img"] = r[0], r[3], r[4], r[5]
            return r
        _C.rasterize_gaussians = spy
        try:
            color, radii = GaussianRasterizer(settings._replace(debug=debug) if debug else settings)(means2D=means2D, **p)
        finally:
            _C.rasterize_gaussians = orig
        color.backward(dpix * scale)
        torch.cuda.synchronize()
        return color.detach(), radii, {k: v.grad for k, v in p.items()}, means2D.grad, cap

    color, radii, grads, g2d, cap = run(1.0)
    # the list structure twice: of the default run (tiles a splat provably misses are left out of the lists, csrc/gsr_rect_trim.h)
    # and of a run that bins every tile of every rectangle like the reference (GSR_DEBUG_NO_TRIM): same image, bit for bit
    color0, radii0, _, _, cap0 = run(1.0, _C.DEBUG_NO_TRIM)
    assert torch.equal(color, color0) and torch.equal(radii, radii0), "the image must not notice what the binning leaves out"
    listed = {}
    for whole, (cap_k, radii_k) in ((False, (cap, radii)), (True, (cap0, radii0))):
        listed[whole] = _list_structure(cap_k, radii_k, P, W, H, T, dev, whole)
    assert listed[True] == cap["R"] and listed[False] <= listed[True]
    line = f"[{name}] instances listed: {listed[False]} of {listed[True]} ({listed[False] / max(listed[True], 1):.3f}) -- the rest lie in tiles their splat provably misses"
    print(line)
    util.parity_log(line)
    R = cap["R"]
    il = _C.image_layout(W, H)
    u32 = lambda buf, off, n: buf[off:off + 4 * n].view(torch.int32)
    lens = (lambda r: r[:, 1] - r[:, 0])(u32(cap["img"], il.ranges, 2 * T).view(T, 2).to(torch.int64))
    final_T = cap["img"][il.final_T:il.final_T + 4 * W * H].view(torch.float32)
    assert bool(torch.isfinite(color).all()) and float(final_T.min()) >= 1e-4 * (1 - 1e-6) and float(final_T.max()) <= 1.0
    n_contrib = u32(cap["img"], il.n_contrib, W * H).to(torch.int64).view(H, W)
    ty, tx = torch.arange(H, device=dev) // 16, torch.arange(W, device=dev) // 16
    assert bool((n_contrib <= lens[(ty[:, None] * ((W + 15) // 16) + tx[None, :])]).all())
    for k, v in grads.items():
        assert bool(torch.isfinite(v).all()), k
    assert bool((grads["means3D"][radii == 0] == 0).all()) and bool((grads["shs"][radii == 0] == 0).all())
    assert bool((g2d[:, 2] == 0).all())
    # bitwise determinism (no atomics anywhere on the path)
    color2, radii2, grads2, g2d2, _ = run(1.0)
    assert torch.equal(color, color2) and torch.equal(radii, radii2) and torch.equal(g2d, g2d2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), f"{k} differs between two identical runs"
    if check_linearity:  # scaling dL/dpix by a power of two scales every gradient exactly
        _, _, grads4, g2d4, _ = run(4.0)
        assert torch.equal(g2d4, g2d * 4.0)
        for k in grads:
            assert torch.equal(grads4[k], grads[k] * 4.0), k
    return R


def test_c3_headline_workload_properties():
    _need_gpu()
    R = _properties("C3")
    assert abs(R - 9.16e6) / 9.16e6 < 0.01  # R measured with the reference's own preprocess


def test_c5_6m_gaussians_4k_properties():
    _need_gpu()
    R = _properties("C5", check_linearity=False)
    assert abs(R - 7.14e7) / 7.14e7 < 0.02
