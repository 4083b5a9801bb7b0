"""GPU: the backward blend takes its band masks from the forward blend (csrc/render_forward.hip, csrc/render_backward.hip).  The
forward stores gsr_tile_band_mask of every list position it stages as one byte (gsr_binning_layout.band_masks); the backward
loads that byte with the position's id, stages the position with it, and gathers the records of the positions whose byte is not
zero only.  GSR_DEBUG_RECOMPUTE_BANDS makes the backward compute the masks from the records as it used to; GSR_DEBUG_NO_CULL
does not consult the array.

Every case gets four checks: (i) the oracle / the path's reference composition with the existing bars of the suite it belongs
to, (ii) default against GSR_DEBUG_RECOMPUTE_BANDS: every gradient byte for byte, (iii) default against GSR_DEBUG_NO_CULL: every
gradient byte for byte, (iv) two runs byte for byte.

The invariants pinned here: the backward never reads a byte the forward did not write (the blob pre-filled with 0x00 and with
0xFF gives the same gradients, although the forward leaves the tail of the list unwritten); a cleared band bit is a band the
float64 footprint does not reach; mixed debug flags between the two calls; a backward run twice over one forward state and over
a state restored from copies of the blobs."""
import ctypes

import numpy as np
import pytest
import torch

import gsr_scene
import util
from test_backward_one_band_gpu import DEV, FOVX, GRADS, UNIT, _maps, _rows_hit, _same_bits, _tile_scene
from test_parity_gpu import check_forward, check_grads

pytestmark = pytest.mark.gpu
_cache = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _four_checks(scene, cam, D, seed, base=0, fragile_cap=0.02):
    """base: bits of the debug mask that every run of the case carries (e.g. the binning path)."""
    from diff_gaussian_rasterization import _C
    o = util.oracle_forward(scene, cam, D)
    assert (o["fragile"] != 0).mean() <= fragile_cap, "too many fragile pixels: choose another seed"
    dpix = util.fragile_free_dpix(o, cam, seed=seed)
    h = util.hip_forward_backward(scene, cam, D, dpix, debug=base)
    check_forward(h, o, cam)                                   # (i)
    check_grads(h, o, dpix, GRADS)
    for label, extra in (("masks stored / recomputed", _C.DEBUG_RECOMPUTE_BANDS),   # (ii)
                         ("cull on / off", _C.DEBUG_NO_CULL),                       # (iii)
                         ("two runs", 0)):                                          # (iv)
        h2 = util.hip_forward_backward(scene, cam, D, dpix, debug=base | extra)
        _same_bits(h["color"], h2["color"], f"color, {label}")
        for k in h["grads"]:
            _same_bits(h["grads"][k], h2["grads"][k], f"{k}, {label}")
        if extra != _C.DEBUG_NO_CULL:   # (dL_dconic and the other internals: the sign of a zero may differ without the cull)
            for k in h["raw_grads"]:
                _same_bits(h["raw_grads"][k], h2["raw_grads"][k], f"raw {k}, {label}")
    return o, h, dpix


class _Abi:
    """One forward through the C ABI with blobs of this test's own (tests/test_boundary_gpu.py does the same), then any number of
    backward calls over that state.  fill: every byte of the binning blob before the forward; the debug masks per call."""

    def __init__(self, scene, cam, D, fwd_debug=0, fill=None, pre_debug=None):
        from diff_gaussian_rasterization import _C
        self.C, self.L = _C, _C.lib()
        L = self.L
        self.scene, self.cam, self.D = scene, cam, D
        self.P, self.W, self.H = scene.means3D.shape[0], cam.image_width, cam.image_height
        self.M = scene.shs.shape[1]
        P, W, H = self.P, self.W, self.H
        self.st = st = util.hip_settings(scene, cam, D, DEV)
        self.t = t = {k: getattr(scene, k).to(DEV).contiguous() for k in ("means3D", "shs", "opacities", "scales", "rotations")}
        byte = dict(dtype=torch.uint8, device=DEV)
        self.geom = torch.empty(L.gsr_geometry_bytes(P), **byte)
        self.img = torch.empty(L.gsr_image_bytes(W, H), **byte)
        self.color = torch.empty(3, H, W, device=DEV)
        R = ctypes.c_int64(0)
        self.stream = torch.cuda.current_stream(DEV).cuda_stream
        ptr = self.ptr
        pre = fwd_debug if pre_debug is None else pre_debug
        _C._check(L.gsr_forward_preprocess(P, D, self.M, W, H, ptr(t["means3D"]), ptr(t["shs"]), None, ptr(t["opacities"]), ptr(t["scales"]), 1.0,
                                           ptr(t["rotations"]), None, ptr(st.viewmatrix), ptr(st.projmatrix), ptr(st.campos), st.tanfovx,
                                           st.tanfovy, 0, None, ptr(self.geom), ctypes.byref(R), self.stream, pre))
        self.R = R = int(R.value)
        self.binning = torch.empty(L.gsr_binning_bytes(P, R, W, H), **byte)
        if fill is not None:
            self.binning.fill_(fill)
        _C._check(L.gsr_forward_render(P, R, W, H, ptr(st.bg), None, ptr(self.geom), ptr(self.binning), ptr(self.img), ptr(self.color), self.stream,
                                       fwd_debug))
        torch.cuda.synchronize()
        self.img_after_forward = self.img.clone()

    @staticmethod
    def ptr(x):
        return x.data_ptr()

    def backward(self, dpix, debug=0, state=None):
        """-> the six gradients as numpy arrays.  state: (geom, binning, img) to run over instead of this forward's own."""
        P, ptr, st, t = self.P, self.ptr, self.st, self.t
        geom, binning, img = state or (self.geom, self.binning, self.img)
        f32 = dict(dtype=torch.float32, device=DEV)
        g = dict(dL_dmeans2D=torch.zeros(P, 3, **f32), dL_dopacity=torch.zeros(P, 1, **f32), dL_dmeans3D=torch.zeros(P, 3, **f32),
                 dL_dsh=torch.zeros(P, self.M, 3, **f32), dL_dscales=torch.zeros(P, 3, **f32), dL_drotations=torch.zeros(P, 4, **f32))
        scratch = torch.empty(max(16, self.L.gsr_backward_scratch_bytes(P, self.R)), dtype=torch.uint8, device=DEV)
        d = dpix.to(DEV).contiguous()
        self.C._check(self.L.gsr_backward(P, self.D, self.M, self.R, self.W, self.H, ptr(st.bg), ptr(t["means3D"]), ptr(t["shs"]), None, ptr(t["scales"]),
                                          1.0, ptr(t["rotations"]), None, ptr(st.viewmatrix), ptr(st.projmatrix), ptr(st.campos), st.tanfovx,
                                          st.tanfovy, None, ptr(geom), ptr(binning), ptr(img), ptr(scratch), ptr(d), ptr(g["dL_dmeans2D"]), None,
                                          ptr(g["dL_dopacity"]), None, ptr(g["dL_dmeans3D"]), None, ptr(g["dL_dsh"]), ptr(g["dL_dscales"]),
                                          ptr(g["dL_drotations"]), self.stream, debug))
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in g.items()}

    def tiles(self):
        """-> (list lengths, walked positions min(length, tile_max_contrib), first list position) per tile, after the forward"""
        il = self.C.image_layout(self.W, self.H)
        T = ((self.W + 15) // 16) * ((self.H + 15) // 16)
        img = self.img_after_forward.cpu().numpy()
        rng = img[il.ranges:il.ranges + 8 * T].view(np.uint32).reshape(T, 2).astype(np.int64)
        tmc = img[il.tile_max_contrib:il.tile_max_contrib + 4 * T].view(np.uint32).astype(np.int64)
        lens = rng[:, 1] - rng[:, 0]
        return lens, np.minimum(lens, tmc), rng[:, 0]

    def masks(self):
        """-> (the band-mask bytes [R], point_list [R]) as the forward left them"""
        bl = self.C.binning_layout(self.P, self.R, self.W, self.H)
        b = self.binning.cpu().numpy()
        assert bl.tile_keys_alt + self.R <= bl.band_masks and bl.band_masks + self.R <= bl.sort_table, "the masks lie outside tile_keys_alt"
        return b[bl.band_masks:bl.band_masks + self.R].copy(), b[bl.point_list:bl.point_list + 4 * self.R].view(np.uint32).copy()

    def dispatch(self, img, extra):
        """the valid entries of the blend's dispatch list in `img` (T + extra entries)"""
        il = self.C.image_layout(self.W, self.H)
        T = ((self.W + 15) // 16) * ((self.H + 15) // 16)
        v = img.cpu().numpy()[il.tile_order:il.tile_order + 4 * (T + extra)].view(np.uint32)
        return v[v != 0xFFFFFFFF]


def _same_grads(a, b, what):
    for k in a:
        _same_bits(a[k], b[k], f"{k}, {what}")


def _sound(abi, o):
    """Mask soundness on a one-tile scene: for every walked position, a cleared band bit is a band that the float64 footprint of
    the listed Gaussian (test_backward_one_band_gpu._rows_hit, from the oracle's mean, conic and opacity) does not reach.
    -> the walked positions' bytes"""
    assert abi.W <= 16 and abi.H <= 16
    lens, walked, start = abi.tiles()
    m, plist = abi.masks()
    rows = _rows_hit(o, abi.W, abi.H)
    n = int(walked[0])
    for i in range(n):
        reached = {int(r) // 4 for r in rows[int(plist[start[0] + i])]}
        for k in range(4):
            assert (m[start[0] + i] >> k) & 1 or k not in reached, \
                f"position {i} (Gaussian {plist[start[0] + i]}): band {k} is cleared in the stored mask {m[start[0] + i]:#x} but rows {sorted(reached)} are reached"
        assert m[start[0] + i] < 16
    return m[start[0]:start[0] + n]


# ---- batch seams ----------------------------------------------------------------------------------------------------------
def _empties(n):
    """The list positions given an empty mask: the first and last lane of a batch and both sides of a batch boundary, as the forward
    counts its batches (from position 0) and as the backward does (from the last walked position, n - 1, which is a contributor and
    so cannot be empty itself)."""
    e = {0, 63, 64, 127, 128, n - 64, n - 65, n - 128, n - 129, 5, n - 7}
    return sorted(p for p in e if 0 <= p < n - 1)


def _seam_scene(n):
    """_tile_scene's faint small Gaussians on one tile, in list order by construction (depth grows with the index); the Gaussians at
    _empties(n) have opacity 0.002 < 1 / 255, so that their mask is empty wherever they lie; the last one is a plain contributor."""
    scene, cam = _tile_scene(n, 3)
    means, opac, scales = scene.means3D.clone(), scene.opacities.clone(), scene.scales.clone()
    means[:, 2] = -0.5 + torch.arange(n, dtype=torch.float32) / n
    opac[_empties(n)] = 0.002
    means[n - 1, :2] = 0.0
    opac[n - 1], scales[n - 1] = 0.1, torch.tensor([0.03, 0.02, 0.03])
    return scene._replace(means3D=means.contiguous(), opacities=opac.contiguous(), scales=scales.contiguous()), cam


@pytest.mark.parametrize("trim", ["whole_lists", "trimmed_lists"])
@pytest.mark.parametrize("n", [64, 65, 128, 129])
def test_batch_seams(n, trim):
    """One tile with n listed instances, the empty masks at the seams of the batches of 64.  whole_lists (GSR_DEBUG_NO_TRIM in every
    run): the binning lists every Gaussian like the reference, so the list positions are the indices and the stored bytes are read
    back at them.  trimmed_lists: the default binning may leave the empty ones out; the four checks alone."""
    _need_gpu()
    from diff_gaussian_rasterization import _C
    scene, cam = _seam_scene(n)
    base = _C.DEBUG_NO_TRIM if trim == "whole_lists" else 0
    o, h, dpix = _four_checks(scene, cam, 2, seed=n, base=base)
    if trim != "whole_lists":
        return
    abi = _Abi(scene, cam, 2, fwd_debug=base)
    lens, walked, start = abi.tiles()
    assert int(lens[0]) == n and int(walked[0]) == n, f"{lens[0]} listed, {walked[0]} walked: not the {n} intended"
    assert np.array_equal(abi.masks()[1][:n], np.arange(n)), "the list is not in index order"
    m = _sound(abi, o)
    empty = set(_empties(n))
    for i in range(n):
        assert (m[i] == 0) == (i in empty), f"position {i}: stored mask {m[i]:#x}, empty positions {sorted(empty)}"
    _same_grads(abi.backward(dpix, base), abi.backward(dpix, base | _C.DEBUG_RECOMPUTE_BANDS), "C ABI, masks stored / recomputed")


# ---- early end ------------------------------------------------------------------------------------------------------------
def _early_end_scene(nfirst=70, nopaque=30, nbehind=150, D=2):
    """70 faint small Gaussians in front, then 30 wide near-opaque ones that finish every pixel of the tile inside the forward's
    second batch, then 150 faint ones behind them that the forward never stages: it breaks out before its third batch."""
    n = nfirst + nopaque + nbehind
    scene, cam = _tile_scene(n, 5, D=D)
    means, opac, scales = scene.means3D.clone(), scene.opacities.clone(), scene.scales.clone()
    means[:, 2] = -0.5 + torch.arange(n, dtype=torch.float32) / n
    px = UNIT / 8   # one pixel in world units at z = 0
    g = torch.Generator().manual_seed(77)
    a, b = nfirst, nfirst + nopaque
    means[a:b, :2] = (torch.rand(nopaque, 2, generator=g) - 0.5) * 6 * px
    opac[a:b] = 0.99
    scales[a:b] = torch.tensor([12 * px, 10 * px, 0.01])
    rot = torch.zeros(n, 4)
    rot[:, 0] = 1.0
    return scene._replace(means3D=means.contiguous(), opacities=opac.contiguous(), scales=scales.contiguous(), rotations=rot), cam


def test_early_end_reads_no_unwritten_mask():
    """The first invariant.  The forward stops staging once every pixel is done, so the masks of the list's tail are never written:
    they hold whatever the blob held.  The backward walks to tile_max_contrib, inside the last batch the forward staged, and must
    read nothing beyond that batch: with the whole binning blob pre-filled with 0x00 and with 0xFF the gradients are the same
    bytes."""
    _need_gpu()
    from diff_gaussian_rasterization import _C
    scene, cam = _early_end_scene()
    o, h, dpix = _four_checks(scene, cam, 2, seed=13, base=_C.DEBUG_NO_TRIM)
    grads = {}
    for fill in (0x00, 0xFF):
        abi = _Abi(scene, cam, 2, fwd_debug=_C.DEBUG_NO_TRIM, fill=fill)
        lens, walked, start = abi.tiles()
        assert int(lens[0]) == 250 and 64 < int(walked[0]) <= 128, f"{lens[0]} listed, {walked[0]} walked: the forward does not end inside its second batch"
        m = abi.masks()[0]
        assert bool((m[128:250] == fill).all()), "the forward wrote masks of batches it did not stage: the case does not test the invariant"
        assert bool((m[:128] < 16).all()), "a staged position's mask was not written"
        _sound(abi, o)
        grads[fill] = abi.backward(dpix, _C.DEBUG_NO_TRIM)
        _same_grads(grads[fill], abi.backward(dpix, _C.DEBUG_NO_TRIM | _C.DEBUG_RECOMPUTE_BANDS), f"fill {fill:#x}, masks stored / recomputed")
    _same_grads(grads[0x00], grads[0xFF], "blob pre-filled with 0x00 / 0xFF")
    for k in grads[0x00]:
        _same_bits(grads[0x00][k], h["grads"][k].reshape(grads[0x00][k].shape), f"{k}, C ABI / autograd surface")


# ---- cut images -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(40, 24), (17, 33)])
def test_images_cut_by_their_edge(W, H):
    """40x24: the lower tiles hold bands 0 and 1 only, the right ones are 8 pixels wide.  17x33: the right tiles are one pixel wide,
    the lowest ones one row high -- whole bands lie outside the image."""
    _need_gpu()
    scene, cam = _tile_scene(60, 1, W, H)
    _four_checks(scene, cam, 2, seed=7)


# ---- heavy tile -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", ["split", "no_split"])
def test_heavy_tile(split):
    """test_absgrad_gpu._heavy_scene: a strip of 64 tiles with a low-opacity blob of 1 300 small Gaussians on one of them.  The forward
    hands that tile out as four band waves (all four store the masks), the backward walks it in depth segments (each reads its own
    stretch of them); with GSR_DEBUG_NO_SPLIT one forward wave blends it."""
    _need_gpu()
    from diff_gaussian_rasterization import _C
    from test_absgrad_gpu import _heavy_scene
    scene, cam, D = _heavy_scene()
    base = _C.DEBUG_NO_SPLIT if split == "no_split" else 0
    o, h, dpix = _four_checks(scene, cam, D, seed=5, base=base)
    abi = _Abi(scene, cam, D, fwd_debug=base)
    lens, walked, start = abi.tiles()
    T = lens.shape[0]
    assert T == 64 and int(lens.max()) >= 640 and int(lens.max()) >= 2 * lens.mean() and int(walked.max()) >= 1024, \
        f"longest list {lens.max()} (mean {lens.mean():.1f}), deepest walk {walked.max()}: not a heavy tile"
    fwd = abi.dispatch(abi.img_after_forward, 3 * min(2048, T // 4))
    nband = int((fwd >> 28 > 0).sum())
    assert nband == (0 if base else 4), f"{nband} band entries in the forward's dispatch list"
    g = abi.backward(dpix, base)
    bwd = abi.dispatch(abi.img, min(4096, T // 2))
    nseg = int((bwd >> 28 > 0).sum())
    assert (nseg == 0) if base else (nseg >= 2), f"{nseg} depth-segment entries in the backward's dispatch list"
    for k in g:
        _same_bits(g[k], h["grads"][k].reshape(g[k].shape), f"{k}, C ABI / autograd surface")
    _same_grads(g, abi.backward(dpix, base | _C.DEBUG_RECOMPUTE_BANDS), "C ABI, masks stored / recomputed")


# ---- flag mixes, replay ---------------------------------------------------------------------------------------------------
def _tile70():
    if "tile70" not in _cache:
        _cache["tile70"] = _tile_scene(70, 0)
    return _cache["tile70"]


def test_flag_mixes_between_the_two_calls():
    """A forward with GSR_DEBUG_NO_CULL leaves 0xF in every staged byte, which a default backward then reads; a default forward
    followed by a GSR_DEBUG_NO_CULL backward does not consult the array.  Both give the bytes of default / default."""
    _need_gpu()
    from diff_gaussian_rasterization import _C
    scene, cam = _tile70()
    o = util.oracle_forward(scene, cam, 2)
    dpix = util.fragile_free_dpix(o, cam, seed=4)
    plain = _Abi(scene, cam, 2)
    want = plain.backward(dpix)
    lens, walked, start = plain.tiles()
    m = _sound(plain, o)
    assert int(walked[0]) > 64 and 0 < int((m != 0xF).sum()), "no mask with a cleared band: the mix would show nothing"
    _same_grads(want, plain.backward(dpix, _C.DEBUG_NO_CULL), "default forward, NO_CULL backward")
    off = _Abi(scene, cam, 2, fwd_debug=_C.DEBUG_NO_CULL, pre_debug=0, fill=0x00)
    assert torch.equal(off.color, plain.color)
    moff = off.masks()[0]
    n = int(off.tiles()[1][0])
    assert n == int(walked[0]) and bool((moff[:n] == 0xF).all()), "a NO_CULL forward must leave 0xF at every staged position"
    _same_grads(want, off.backward(dpix), "NO_CULL forward, default backward")
    _same_grads(want, off.backward(dpix, _C.DEBUG_RECOMPUTE_BANDS), "NO_CULL forward, RECOMPUTE_BANDS backward")
    _same_grads(want, off.backward(dpix, _C.DEBUG_NO_CULL), "NO_CULL forward, NO_CULL backward")


def test_backward_twice_and_over_a_restored_state():
    """The masks belong to the forward state: a second backward over it, with another dL/dpix in between, and one over copies of
    the three blobs that went through host memory (what a debug snapshot restores) give the first one's bytes."""
    _need_gpu()
    scene, cam = _tile70()
    o = util.oracle_forward(scene, cam, 2)
    dpix = util.fragile_free_dpix(o, cam, seed=4)
    abi = _Abi(scene, cam, 2)
    first = abi.backward(dpix)
    abi.backward(util.fragile_free_dpix(o, cam, seed=5))
    _same_grads(first, abi.backward(dpix), "second backward over one forward state")
    restored = tuple(torch.from_numpy(b.cpu().numpy().copy()).to(DEV) for b in (abi.geom, abi.binning, abi.img))
    _same_grads(first, abi.backward(dpix, state=restored), "backward over a restored state")


# ---- variants -------------------------------------------------------------------------------------------------------------
def _switches():
    from diff_gaussian_rasterization import _C
    return (("masks stored / recomputed", _C.DEBUG_RECOMPUTE_BANDS), ("cull on / off", _C.DEBUG_NO_CULL), ("two runs", 0))


def test_tile70_tile_sort():
    """The 70-Gaussian tile through the instance emission + tile sort (GSR_DEBUG_TILE_SORT to both forward calls): the masks live in
    the sort's ping-pong buffer, which is dead by the time the forward blend runs."""
    _need_gpu()
    from diff_gaussian_rasterization import _C
    scene, cam = _tile70()
    _four_checks(scene, cam, 2, seed=70, base=_C.DEBUG_TILE_SORT)


def test_tile70_depth_and_alpha():
    """... through GaussianRasterizer(depth_alpha="depth") against the two-pass composition, with test_depth_alpha_gpu.py's bars."""
    _need_gpu()
    import test_depth_alpha_gpu as da
    scene, cam = _tile70()
    dpix, dD, dA = _maps(11, 16, 16)
    f = da.fused(scene, cam, 2, "depth", dpix, dD, dA)
    r = da.two_pass(scene, cam, 2, "depth", dpix, dD, dA)
    da.check_forward(f, r)
    da.check_grads(f[4], r[3], da.two_pass(scene, cam, 2, "depth", dpix, dD, dA, split=True)[3], label="forward masks tile70/depth")
    for label, debug in _switches():
        f2 = da.fused(scene, cam, 2, "depth", dpix, dD, dA, debug=debug)
        for a, b in zip(f[:4], f2[:4]):
            _same_bits(a.cpu().numpy(), b.cpu().numpy(), f"outputs, {label}")
        for k in f[4]:
            _same_bits(f[4][k].cpu().numpy(), f2[4][k].cpu().numpy(), f"{k}, {label}")


@pytest.mark.parametrize("variant", ["absgrad", "absgrad_invdepth"])
def test_tile70_absgrad(variant):
    """... through absgrad, alone and together with the depth-and-alpha maps, against the float64 per-pixel terms with
    test_absgrad_gpu.py's bar."""
    _need_gpu()
    import test_absgrad_gpu as ab
    scene, cam = _tile70()
    o = util.oracle_forward(scene, cam, 2)
    dpix = util.fragile_free_dpix(o, cam, seed=3)
    kw, run_kw, dL = {}, {}, dpix
    if variant == "absgrad_invdepth":
        g = torch.Generator().manual_seed(5)
        dL = (dpix, torch.randn(16, 16, generator=g) * (dpix[0] != 0), torch.randn(16, 16, generator=g) * (dpix[0] != 0))
        kw["depth_mode"], run_kw["depth_alpha"] = "invdepth", "invdepth"
    ref, signed, d32 = ab._terms(scene, cam, dL, D=2, o=o, **kw)
    a = ab._run(scene, cam, dL, "both", D=2, **run_kw)
    ab._check(a["abs_mean2D"], ref, d32, f"forward masks tile70 {variant}")
    for label, debug in _switches():
        b = ab._run(scene, cam, dL, "both", D=2, debug=debug, **run_kw)
        ab._same_everything(a, b)
        _same_bits(a["abs_mean2D"].cpu().numpy(), b["abs_mean2D"].cpu().numpy(), f"abs_mean2D, {label}")
        _same_bits(a["accum"].cpu().numpy(), b["accum"].cpu().numpy(), f"accum, {label}")


def test_tile70_antialiased():
    """... with anti-aliasing, against the composition of test_antialias_gpu.py with its bars."""
    _need_gpu()
    import test_antialias_gpu as aa
    scene, cam = _tile70()
    aa._check(scene, cam, 2, "sh", "forward masks tile70/aa")
    dpix, _, _ = aa._dpix(1, 16, 16)
    f, g = aa.fused(scene, cam, 2, "sh", dpix)
    for label, debug in _switches():
        f2, g2 = aa.fused(scene, cam, 2, "sh", dpix, debug=debug)
        for a, b in zip(f, f2):
            _same_bits(a.cpu().numpy(), b.cpu().numpy(), f"outputs, {label}")
        for k in g:
            _same_bits(g[k].cpu().numpy(), g2[k].cpu().numpy(), f"{k}, {label}")


# ---- seeded random scenes ---------------------------------------------------------------------------------------------------
def _random_scene(seed):
    rng = np.random.default_rng(300 + seed)
    P = int(rng.integers(300, 1200))
    W, H = int(rng.integers(16, 65)), int(rng.integers(16, 65))
    D = int(rng.integers(0, 4))
    scene = gsr_scene.make_scene(P, float(rng.uniform(-3.5, -1.5)), sh_degree=D, seed=seed)
    cam = gsr_scene.ring_camera(W, H, int(rng.integers(0, 8)), 8, radius=float(rng.uniform(0.5, 4.5)))
    return scene, cam, D


@pytest.mark.parametrize("seed", range(4))
def test_random_scenes(seed):
    """Cameras inside and outside the cloud, odd image sizes up to 64x64, up to 1 200 Gaussians; the seeds were checked against the
    oracle on the CPU: at most 2 % of the pixels are fragile (the cap of test_backward_one_band_gpu.py, asserted by _four_checks)."""
    _need_gpu()
    scene, cam, D = _random_scene(seed)
    _four_checks(scene, cam, D, seed=seed)
