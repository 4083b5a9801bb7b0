"""GPU: the depth sort and the binning with a count exactly on, one below and one above every fixed size the kernels are built
from ("Seams of the binning chain"; fixtures and numpy reference: tests/binning_cases.py, their conditions:
tests/test_binning_seams_cpu.py).

Everything compared here is an integer or a bit pattern: the depth order is numpy's stable argsort of the depth bits, the instance
list, its keys and the tile ranges are the reference's duplicateWithKeys + SortPairs + identifyTileRanges restated in numpy on the
run's own depth bits and rectangles (the inputs of the chain under test), less the instances the trim words name on the default
path.  The only tolerances are the existing oracle bars of check_forward / check_grads where a case has no second GPU path (D4, F).

  A  depth order at count seams (64, 256, 1 024, 16 384, 65 536; 2 048 culled), bucket sort and radix passes
  B  bucket capacities of the bucket sort (2 048 in LDS, 12 288 in registers, part counts, next-digit levels, top_shift = 0)
  C  column pairs: segments of both passes, column-aligned workgroups, longest group sequences, trim-word geometry
  D  instance emission + tile sort: range kernel, radix block and chunk seams, empty tile runs, pass-count parity, u32 tile ids
  E  the three-level offset walk of both column-pair passes (more than 64 chunks of 64 blocks), and the radix depth passes on both
     sides of their switch from 4 to 16 keys per thread
  F  tile order on both sides of the 9 216 tiles it keeps in registers"""
import numpy as np
import pytest
import torch

import binning_cases as bc
import util

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _grid(cam):
    return (cam.image_width + 15) // 16, (cam.image_height + 15) // 16


def _forward(c, debug):
    """One forward through the binding with precomputed colours at degree 0 -> (R, color, radii, geom, binning, img) and the device inputs."""
    from diff_gaussian_rasterization import _C
    dev = torch.device("cuda:0")
    st = util.hip_settings(c.scene, c.cam, 0, dev)
    e = torch.empty(0, device=dev)
    t = {k: getattr(c.scene, k).to(dev) for k in ("means3D", "opacities", "scales", "rotations")}
    t["colors"] = c.colors.to(dev)
    out = _C.rasterize_gaussians(st.bg, t["means3D"], t["colors"], t["opacities"], t["scales"], t["rotations"], 1.0, e, st.viewmatrix,
                                 st.projmatrix, st.tanfovx, st.tanfovy, st.image_height, st.image_width, e, 0, st.campos, False, debug)
    torch.cuda.synchronize()
    return out, st, t


def _run(c, debug=0):
    from diff_gaussian_rasterization import _C
    (R, color, radii, geom, binning, img), _, _ = _forward(c, debug)
    o = util.unpack_state(dict(R=R, geom=geom, binning=binning, img=img), c.P, c.cam.image_width, c.cam.image_height,
                          tile_sort=bool(debug & _C.DEBUG_TILE_SORT))
    o["color"], o["radii"], o["R"] = color.cpu().numpy(), radii.cpu().numpy(), R
    return o


def _reference(c, h, name=None):
    """The numpy reference on the run's own depth bits and rectangles; for the fixtures the CPU file covers, those are also the oracle's."""
    gx, gy = _grid(c.cam)
    rect = bc.rect_of_state(h["rect"], h["tiles_touched"])
    if name is not None:
        o = bc.oracle_state(name)
        vis = o["radii"] > 0
        assert np.array_equal(h["depth_bits"], np.where(vis, o["depths"].view(np.uint32), bc.CULLED)), f"{name}: depth bits differ from the oracle's"
        assert np.array_equal(rect, bc.rect_of_oracle(o)), f"{name}: rectangles differ from the oracle's"
        assert h["R"] == o["num_rendered"]
    return bc.reference_binning(rect, h["depth_bits"], gx, gy)


def _check_depth_order(h, label):
    bits = h["depth_bits"]
    want = bc.reference_depth_order(bits)
    np.testing.assert_array_equal(h["perm"], want, err_msg=f"{label}: order")
    np.testing.assert_array_equal(h["sorted_depth_keys"], bits[want], err_msg=f"{label}: sorted keys")
    tt = h["tiles_touched"].astype(np.int64)
    np.testing.assert_array_equal(h["slot_base"][tt > 0], (np.cumsum(tt) - tt)[tt > 0].astype(np.uint32), err_msg=f"{label}: slot_base")
    assert h["slots_in_index_order"] == 1, label


def _depth_case(name, bucket_condition=False):
    from diff_gaussian_rasterization import _C
    c = bc.case(name)
    gx, gy = _grid(c.cam)
    a = _run(c, 0)
    b = _run(c, _C.DEBUG_RADIX_DEPTH)
    assert np.array_equal(a["depth_bits"], c.bits) and np.array_equal(b["depth_bits"], c.bits), f"{name}: the depth bits are not the chosen ones"
    if bucket_condition:   # the fixture condition, asserted on the run's own keys before anything is compared
        db = bc.depth_buckets(a["depth_bits"])
        assert db["top_shift"] == c.expect["top_shift"] and db["range"] == c.expect["range"]
        if "slab" in c.expect:
            assert int(db["sizes"][c.expect["slab"][0]]) == c.expect["slab"][1]
    want = _reference(c, a, name)
    tt = a["tiles_touched"].astype(np.int64)
    assert np.array_equal(tt[tt > 0], np.resize([1, 2, 4], c.P)[tt > 0])   # centres, seams, corners in rotation: the prefix is not the identity
    for h, path in ((a, "bucket"), (b, "radix")):
        _check_depth_order(h, f"{name}: {path}")
        bc.check_lists(h, bc.trimmed(want, h["rshape"], gx, gy), f"{name}: {path}")
    for k in ("point_list", "ranges", "color"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name}: {k} differs between the two depth sorts")


@pytest.mark.parametrize("name", bc.A_NAMES)
def test_A_depth_order_at_count_seams(name):
    _need_gpu()
    _depth_case(name)


@pytest.mark.parametrize("name", bc.B_NAMES)
def test_B_bucket_capacities(name):
    _need_gpu()
    _depth_case(name, bucket_condition=True)


@pytest.mark.parametrize("name", bc.C_NAMES)
def test_C_column_pairs(name):
    _need_gpu()
    from diff_gaussian_rasterization import _C
    c = bc.case(name)
    gx, gy = _grid(c.cam)
    full = _run(c, _C.DEBUG_NO_TRIM)
    dflt = _run(c, 0)
    tsort = _run(c, _C.DEBUG_TILE_SORT)
    assert _C.binning_layout(c.P, full["R"], c.cam.image_width, c.cam.image_height).column_pairs == 1
    want = _reference(c, full, name)
    assert not full["rshape"][:, 1].any()
    bc.check_lists(full, want, f"{name}: column pairs, every tile")
    bc.check_lists(tsort, want, f"{name}: tile sort")
    bc.check_lists(dflt, bc.trimmed(want, dflt["rshape"], gx, gy), f"{name}: column pairs, trimmed")
    assert len(dflt["point_list"]) <= len(full["point_list"]) == full["R"]
    if name in bc.C5_NAMES:   # the fixture has every shape at both opacities: the faint twins lose tiles, and more than the others
        kept = np.bincount(dflt["point_list"], minlength=c.P)
        big = full["tiles_touched"] > 1
        lo = big & (c.scene.opacities.numpy()[:, 0] < 0.5)
        assert (kept[lo] < full["tiles_touched"][lo]).all() and kept[lo].sum() < kept[big & ~lo].sum()
    for k in ("color", "radii", "final_T", "depth_bits", "rect"):
        assert np.array_equal(dflt[k], full[k]) and np.array_equal(tsort[k], full[k]), f"{name}: {k}"


@pytest.mark.parametrize("name", bc.D_SMALL_NAMES)
def test_D_tile_sort(name):
    _need_gpu()
    from diff_gaussian_rasterization import _C
    c = bc.case(name)
    gx, gy = _grid(c.cam)
    forced = max(gx, gy) <= 256    # beyond 256 tiles per side the library takes this path by itself
    h = _run(c, _C.DEBUG_TILE_SORT if forced else 0)
    bl = _C.binning_layout(c.P, h["R"], c.cam.image_width, c.cam.image_height)
    assert bl.tile_key_bytes == 2 and bool(bl.column_pairs) == forced
    want = _reference(c, h, name)
    assert h["R"] == c.expect["R"]
    bc.check_lists(h, want, name)
    _check_depth_order(h, name)
    if forced:
        d = _run(c, 0)
        for k in ("color", "radii", "final_T"):
            assert np.array_equal(d[k], h[k]), f"{name}: {k}"


def test_D4_u32_tile_ids():
    """65 538 tiles: uint32 tile ids in the emission, three sort passes, the uint32 range kernel.  There is no second GPU path for this
    image, so it is also held against the oracle with the existing bars, with one backward."""
    _need_gpu()
    from diff_gaussian_rasterization import _C
    from test_parity_gpu import check_forward, check_grads
    name = bc.D4_NAME
    c = bc.case(name)
    W, H = c.cam.image_width, c.cam.image_height
    gx, gy = _grid(c.cam)
    assert gx * gy == 65538
    o = bc.oracle_state(name)
    dpix = util.fragile_free_dpix(o, c.cam)
    h = util.hip_forward_backward(c.scene, c.cam, 0, dpix, colors_precomp=c.colors, use_sh=False)
    h["R"] = h["num_rendered"]
    bl = _C.binning_layout(c.P, h["R"], W, H)
    assert bl.tile_key_bytes == 4 and not bl.column_pairs
    want = _reference(c, h, name)
    lens = h["ranges"][:, 1].astype(np.int64) - h["ranges"][:, 0]
    assert lens[65536] >= 20 and lens[65537] >= 20
    assert int((bc.rect_of_state(h["rect"], h["tiles_touched"])[:, 3] == 2).sum()) >= 20
    bc.check_lists(h, want, name)
    _check_depth_order(h, name)
    err = check_forward(h, o, c.cam)
    util.parity_log(f"[{name}] P={c.P} {W}x{H}: R={h['R']}, integer state exact, image max-abs (non-fragile) {err:.3e}")
    print(f"{name}: image max-abs err {err:.3e}")
    check_grads(h, o, dpix, ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dcolors", "dL_dscales", "dL_drotations"], label=name)


def _sliced_state(cap, P, W, H):
    """What group E needs of util.unpack_state's result, sliced out of the state blobs on the device: the whole geometry blob of 4 Mi
    Gaussians is half a gigabyte."""
    from diff_gaussian_rasterization import _C
    gl, il = _C.geometry_layout(P), _C.image_layout(W, H)
    geom, img, binning, R = cap["geom"], cap["img"], cap["binning"], cap["R"]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    u32 = lambda blob, off, n: blob[off:off + 4 * n].cpu().numpy().view(np.uint32)
    status = u32(geom, gl.status, 4)
    in_alt = int(status[2])
    o = dict(depth_sort_result_in_alt=in_alt, slots_in_index_order=int(status[3]), R=R)
    o["perm"] = u32(geom, gl.perm_alt if in_alt else gl.perm, P)
    o["sorted_depth_keys"] = u32(geom, gl.depth_keys_alt if in_alt else gl.depth_keys, P)
    o["depth_bits"] = np.empty(P, np.uint32)
    o["depth_bits"][o["perm"]] = o["sorted_depth_keys"]
    o["tiles_touched"] = u32(geom, gl.tiles_touched, P)
    o["rect"] = u32(geom, gl.rect, 2 * P).reshape(P, 2)
    o["ranges"] = u32(img, il.ranges, 2 * T).reshape(T, 2)
    bl = _C.binning_layout(P, R, W, H)
    assert int(bl.column_pairs)
    o["point_list"] = u32(binning, bl.point_list, R)
    lens = o["ranges"][:, 1].astype(np.int64) - o["ranges"][:, 0]
    assert int(lens.sum()) == R   # (GSR_DEBUG_NO_TRIM: every instance is listed)
    o["keys"] = (np.repeat(np.arange(T, dtype=np.uint64), lens) << np.uint64(32)) | o["depth_bits"][o["point_list"]].astype(np.uint64)
    return o


@pytest.mark.parametrize("name", bc.E_NAMES)
def test_E_three_level_offset_walk(name):
    """4 096 blocks of 1 024 are 64 chunks (two levels of offset tables); one Gaussian more makes 65 (three levels) -- in pass 1 of the
    column pairs (blocks over all pairs) and in pass 2 (column-aligned blocks: the fixture holds exactly 256 Ki pairs per tile column,
    and the extra one opens a block of its own).  Both block counts are asserted on the run's own rectangles first.
    The radix depth passes (csrc/sort.hip; the only depth sort beyond 2 Mi Gaussians) stay two-level at these sizes -- their
    three-level walk needs more than 16.7 M keys and is out of reach here: 4 Mi is the last size they take with 4 keys per thread
    (4 096 blocks, 64 chunks: the fullest two-level table), 4 Mi + 1 the first with 16 (1 025 blocks)."""
    _need_gpu()
    from diff_gaussian_rasterization import _C
    try:
        c = bc.case(name)
        W, H = c.cam.image_width, c.cam.image_height
        (R, color, radii, geom, binning, img), _, _ = _forward(c, _C.DEBUG_NO_TRIM)
        h = _sliced_state(dict(R=R, geom=geom, binning=binning, img=img), c.P, W, H)
        del geom, binning, img, color, radii
        assert R == c.P and h["depth_sort_result_in_alt"] in (0, 1)
        assert np.array_equal(h["depth_bits"], c.bits)
        assert np.array_equal(h["tiles_touched"], np.ones(c.P, np.uint32))
        # the fixture condition: blocks and chunks of both passes from the run's own rectangles
        rect = bc.rect_of_state(h["rect"], h["tiles_touched"])
        assert (rect[:, 2] == 1).all() and (rect[:, 3] == 1).all()
        col_pairs = np.bincount(rect[:, 0], minlength=16)
        assert np.array_equal(col_pairs, c.expect["col_pairs"])
        bk = bc.blocks_and_chunks(col_pairs)
        assert bk["pass1"] == c.expect["pass1"] and bk["pass2"] == c.expect["pass2"], bk
        assert (bk["pass1"][1] > bc.E_CHUNK) == (bk["pass2"][1] > bc.E_CHUNK) == (c.P > 4096 * 1024)   # two levels against three
        assert (c.P <= bc.E_SORT_SMALL_N) == (c.P == 4096 * 1024)                                       # 4 against 16 keys per thread
        want = bc.reference_depth_order(c.bits)
        np.testing.assert_array_equal(h["perm"], want)
        np.testing.assert_array_equal(h["sorted_depth_keys"], c.bits[want])
        bc.check_lists(h, bc.reference_binning(rect, h["depth_bits"], *_grid(c.cam)), name)
    finally:
        bc.case.cache_clear()   # (a quarter of a gigabyte per fixture: not kept for the rest of the session)


def _dispatch_entries(img, il, count):
    v = img[il.tile_order:il.tile_order + 4 * count].view(torch.int32).to(torch.int64).cpu().numpy() & 0xFFFFFFFF
    return v[v != 0xFFFFFFFF]


def _check_dispatch_list(valid, T, bands, label):
    """The list's tile fields are a permutation of all T tiles: every tile once as a whole, or as its four band entries (forward) / its
    depth segments 1 .. n (backward), counted as tests/test_boundary_gpu.py counts them."""
    tile, sub = valid & 0x0FFFFFFF, valid >> 28
    whole = np.sort(tile[sub == 0])
    parts, n_parts = np.unique(tile[sub > 0], return_counts=True)
    assert np.array_equal(np.sort(np.concatenate([whole, parts])), np.arange(T)), f"{label}: the entries' tiles are not all {T} tiles once"
    assert valid.size == T + int((sub > 0).sum()) - parts.size, label
    for t, n in zip(parts, n_parts):
        s = np.sort(sub[(tile == t) & (sub > 0)])
        assert np.array_equal(s, np.arange(1, n + 1)) and (n == 4 if bands else n >= 2), f"{label}: tile {t} has the entries {s}"
    return parts.size


@pytest.mark.parametrize("name", bc.F_NAMES)
def test_F_tile_order(name):
    _need_gpu()
    from diff_gaussian_rasterization import _C
    from test_parity_gpu import check_forward
    c = bc.case(name)
    W, H = c.cam.image_width, c.cam.image_height
    T = c.expect["tiles"]
    il = _C.image_layout(W, H)
    (R, color, radii, geom, binning, img), st, t = _forward(c, 0)
    assert R > 0
    nsplit = _check_dispatch_list(_dispatch_entries(img, il, T + 3 * min(2048, T // 4)), T, True, f"{name}: forward")
    e = torch.empty(0, device=color.device)
    dpix = torch.randn(3, H, W, generator=torch.Generator().manual_seed(2)).to(color.device)
    _C.rasterize_gaussians_backward(st.bg, t["means3D"], radii, t["colors"], t["scales"], t["rotations"], 1.0, e, st.viewmatrix, st.projmatrix,
                                    st.tanfovx, st.tanfovy, dpix, e, 0, st.campos, geom, R, binning, img, False)
    torch.cuda.synchronize()
    ncut = _check_dispatch_list(_dispatch_entries(img, il, T + min(4096, T // 2)), T, False, f"{name}: backward")
    print(f"{name}: {T} tiles, R {R}, {nsplit} split in bands, {ncut} cut in depth")
    if max(_grid(c.cam)) <= 256:
        ts = _run(c, _C.DEBUG_TILE_SORT)
        assert np.array_equal(color.cpu().numpy(), ts["color"]) and np.array_equal(radii.cpu().numpy(), ts["radii"])
    else:
        h = util.hip_forward_backward(c.scene, c.cam, 0, None, colors_precomp=c.colors, use_sh=False)
        assert np.array_equal(h["color"], color.cpu().numpy())
        check_forward(h, bc.oracle_state(name), c.cam)
