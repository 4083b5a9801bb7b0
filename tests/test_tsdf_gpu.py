"""GPU: TSDF fusion and marching tetrahedra (include/gsr_tsdf.h, fused_tsdf.py) against tests/torch_tsdf.py in float64.

Integration, the grids, camera counts and images of torch_tsdf (a lone lane, a full wave and one over it, one brick of 8 x 8 x 4 and one
over it in each axis, several workgroups with a remainder; 1, 3 and 5 cameras in front of, beside and behind the grid; depth maps with
zeros, negatives, NaN, +inf and values beyond depth_trunc; weights with zeros).  Nodes where a decision lies inside the fp32 error of
its own inputs are skipped (tests/test_tsdf_cpu.py caps them at 1 %); every other node is within the reference's derived bound:
    wsum, csum   (C + 1) 2^-24 (|start| + sum |term|): each addition rounds a partial sum
    dsum         the same, plus per term w (E_s / sdf_trunc + 3 * 2^-24 |tsdf|), E_s = 8 * 2^-24 S_z + 2 * 2^-24 (|d| + |p_z|)
Derived, not measured.  Nodes no camera touches keep their bits; a split batch, strided inputs and the packed
records give the bits of the whole contiguous batch.  Canary rows behind every plane and every output.
Extraction, the fields of torch_tsdf through from_planes: V, F and the faces (rotated to begin at their smallest index) equal the
reference's exactly and in order; vertices and colours lie within 4 * 2^-24 of the edge's extent (the larger modulus of the edge's two
ends, per coordinate and per channel): the kernel evaluates in double and rounds once, 2^-24 of the value itself, which is at most the
extent.  The topology checks of the CPU file are repeated on the GPU's own faces.
Extraction without smoothness, against torch_tsdf.mesh_ref_fast (the array form of the reference, which tests/test_tsdf_cpu.py holds
to the loop form bit for bit), with the same assertions and the same bar, plus 0 <= faces < V and the vertices at t = 0 or 1 equal to
the float32 of their node:
    noise at (9, 8, 5) and (33, 17, 9), min_weight 1.0 and 2.0   reaches every (tetrahedron, case) row of the table (the CPU file
        counts them), nodes of value +0 and -0 beside negative ones, and at 2.0 scattered invalid nodes: tetrahedra suppressed beside
        emitting ones in one cell, vertices no face names, nodes without crossings whose cells the face pass does not read, and
        wsum == min_weight (valid) against the float32 below it (invalid)
    noise at (65, 64, 17), 277 count workgroups, all with counts   reaches the plan scan's wave seam: threads 63 | 64, the prefix
        over the wave totals in gsr_tsdf_block_scan<16>
    the seam volume (128, 128, 66), 4 224 count workgroups         reaches the wave seams 63 | 64, 127 | 128 and 255 | 256 with empty
        stretches between them, and the chunk seam 4 095 | 4 096: the second trip of the scan's loop and its 64-bit carry, for V
        and for F, up to the last workgroup that holds a cell
    not reached: the truncation of the bases to 32 bits, which needs more than 2^31 vertices.
Each of these breaks of gsr_tsdf_scan_kernel, built apart and run once on the MI355X, fails exactly the tests named and none that
this file had before them: without the `k < w` prefix in the scan kernel's block scan, the two seam tests; with the bases written
without the carry, the chunk-seam test.  (Without `carry += tot` the totals themselves are 0, and every extraction test fails.)
Measured on the MI355X (this file, printed by the tests):
    integration  largest error / bound over all cases: wsum 0.50, dsum 0.17, csum 0.49
    extraction   vertices 0.24, colours 0.25 of the bar (one rounding)
    noise, seams vertices 0.248, colours 0.249 of the bar; the chunk-seam test takes 0.9 s, 3 to 4 ms of it in _extract (three
                 extractions and the copies), the rest its reference
    end to end   every vertex within 0.860 voxel_size of the analytic sphere (the float64 reference: 0.860)
"""
import ctypes

import numpy as np
import pytest
import torch

import torch_tsdf as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
GUARD = 64          # canary elements behind every plane and output
CANARY = -777.25
_cache = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _padded_plane(values):
    """`values` ((3,) NZ, NY, NX) in front of GUARD canaries in one allocation -> (the plane as a view, the whole buffer)"""
    flat = torch.full((values.size + GUARD,), CANARY, dtype=torch.float32, device=DEV)
    flat[:values.size] = _dev(values).reshape(-1)
    return flat[:values.size].view(values.shape), flat


def _intact(buf):
    return bool((buf[-GUARD:] == CANARY).all())


def _scene(dims, C, image):
    """-> the scene and its float64 reference, computed once and never written to"""
    key = (dims, C, image)
    if key not in _cache:
        s = ref.integration_scene(dims, C, image)
        _cache[key] = (s, ref.integrate_ref(dims, s.origin, s.voxel_size, s.rec, s.depth, s.color, s.weight, wsum0=s.wsum0, dsum0=s.dsum0, csum0=s.csum0))
    return _cache[key]


def _volume(s, color=True):
    import fused_tsdf as ft
    w, wb = _padded_plane(s.wsum0)
    d, db = _padded_plane(s.dsum0)
    c, cb = _padded_plane(s.csum0) if color else (None, None)
    vol = ft.TSDFVolume.from_planes(tuple(float(v) for v in s.origin), float(s.voxel_size), w, d, c, sdf_trunc=ref.SDF_TRUNC, depth_trunc=ref.DEPTH_TRUNC)
    return vol, [b for b in (wb, db, cb) if b is not None]


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("image", ref.IMAGES)
@pytest.mark.parametrize("C", ref.CAMERAS)
@pytest.mark.parametrize("dims", ref.GRIDS)
def test_integration_matches_the_float64_reference(dims, C, image):
    s, r = _scene(dims, C, image)
    nodes = dims[0] * dims[1] * dims[2]
    rec, depth, color, weight = _dev(s.rec), _dev(s.depth), _dev(s.color), _dev(s.weight)
    vol, bufs = _volume(s)
    assert vol.integrate(depth, rec, color=color, weight=weight) is vol
    torch.cuda.synchronize()
    assert all(_intact(b) for b in bufs)
    got_w, got_d, got_c = vol.wsum.reshape(-1).double().cpu().numpy(), vol.dsum.reshape(-1).double().cpu().numpy(), vol.csum.reshape(3, -1).double().cpu().numpy()
    keep = ~r.ambiguous
    assert int((~keep).sum()) <= nodes // 100
    worst = {}
    for name, got, want, bound in (("wsum", got_w, r.wsum, r.bound_w), ("dsum", got_d, r.dsum, r.bound_d), ("csum", got_c, r.csum, r.bound_c)):
        err = np.abs(got - want)[..., keep]
        b = bound[..., keep]
        worst[name] = float((err / np.maximum(b, 1e-300)).max()) if err.size else 0.0
        assert bool((err <= b).all()), (name, worst[name])
    print(f"{dims} C = {C} {image}: error / bound wsum {worst['wsum']:.3f}, dsum {worst['dsum']:.3f}, csum {worst['csum']:.3f} over {int(keep.sum())} nodes; "
          f"{int(r.touched.sum())} touched; pairs skipped {r.skipped}, cut {r.cut}, clamped {r.clamped}")
    if nodes > 1:   # the skip, the cut and the clamp all occur
        assert r.skipped > 0 and r.cut > 0 and r.clamped > 0
    # nodes no camera touches keep their previous bits
    quiet = torch.from_numpy(keep & ~r.touched).to(DEV)
    for plane, before in ((vol.wsum, s.wsum0), (vol.dsum, s.dsum0), (vol.csum[0], s.csum0[0]), (vol.csum[2], s.csum0[2])):
        assert _same(plane.reshape(-1)[quiet], _dev(before).reshape(-1)[quiet])
    changed = torch.from_numpy(keep & r.touched).to(DEV)
    assert bool((vol.wsum.reshape(-1)[changed] > _dev(s.wsum0).reshape(-1)[changed]).all())

    def run(fn, color_planes=True):
        v, b = _volume(s, color_planes)
        fn(v)
        torch.cuda.synchronize()
        assert all(_intact(x) for x in b)
        return v

    def equal(v):
        return _same(v.wsum, vol.wsum) and _same(v.dsum, vol.dsum) and (v.csum is None or _same(v.csum, vol.csum))

    assert equal(run(lambda v: v.integrate(depth, rec, color=color, weight=weight)))                     # two runs, the same bits
    assert equal(run(lambda v: v.integrate(depth[:, None], rec, color=color, weight=weight[:, None])))   # (C,1,H,W)
    assert equal(run(lambda v: v.integrate(depth, rec, weight=weight), color_planes=False))             # without colour planes
    if C > 1:   # a split batch is the whole batch
        k = 2 if C > 2 else 1
        assert equal(run(lambda v: v.integrate(depth[:k], rec[:k], color=color[:k], weight=weight[:k]).integrate(depth[k:], rec[k:], color=color[k:],
                                                                                                               weight=weight[k:])))
        assert equal(run(lambda v: v.integrate(depth[:1], rec[:1], color=color[:1], weight=weight[:1]).integrate(depth[1:], rec[1:], color=color[1:],
                                                                                                               weight=weight[1:])))
    else:       # one camera: (H,W), (1,H,W) and (3,H,W)
        assert equal(run(lambda v: v.integrate(depth[0], rec, color=color[0], weight=weight[0])))
    # strided inputs
    H, W = s.H, s.W
    sd = torch.zeros(C, H, 2 * W, device=DEV)[:, :, ::2]
    sd.copy_(depth)
    sw = torch.zeros(C, 2 * H, W, device=DEV)[:, ::2]
    sw.copy_(weight)
    sc = torch.zeros(C, H, W, 3, device=DEV).permute(0, 3, 1, 2)
    sc.copy_(color)
    srec = torch.zeros(C, 40, device=DEV)[:, ::2]
    srec.copy_(rec)
    assert not sd.is_contiguous() and not sw.is_contiguous() and not sc.is_contiguous() and not srec.is_contiguous()
    assert equal(run(lambda v: v.integrate(sd, srec, color=sc, weight=sw)))


def test_integration_from_a_camera_list_and_the_views_of_the_field():
    """a list of camera objects is packed to the records a packed tensor holds; tsdf() is NaN exactly where weight() is 0"""
    import fused_filter3d as ff
    import fused_tsdf as ft
    import torch_filter3d
    cams = torch_filter3d.ring_cameras(3)   # 64 x 48, looking at the origin from 4 away
    depth = torch.full((3, 48, 64), 3.2, device=DEV)
    a = ft.TSDFVolume((-1.0, -1.0, -1.0), 0.125, (17, 16, 15), device=DEV).integrate(depth, cams)
    b = ft.TSDFVolume((-1.0, -1.0, -1.0), 0.125, (17, 16, 15), device=DEV).integrate(depth, ff.pack_cameras(cams, DEV))
    assert a.wsum.shape == (15, 16, 17) and a.csum.shape == (3, 15, 16, 17) and a.sdf_trunc == 0.5
    assert _same(a.wsum, b.wsum) and _same(a.dsum, b.dsum) and float(a.wsum.max()) >= 1.0 and float(a.csum.abs().max()) == 0.0
    t, w = a.tsdf(), a.weight()
    assert w is a.wsum and t.shape == w.shape and bool((torch.isnan(t) == (w == 0)).all()) and bool((w == 0).any()) and bool((w > 0).any())
    assert float(t[w > 0].max()) <= 1.0 and float(t[w > 0].min()) >= -1.0
    with pytest.raises(RuntimeError, match="camera 0 is 64 x 48"):
        a.integrate(depth[:, :, :32], ff.pack_cameras(cams, DEV))
    a.reset()
    assert float(a.wsum.abs().max()) == 0.0 and float(a.dsum.abs().max()) == 0.0


# ---- extraction ----
def _field(name, dims):
    key = ("field", name, dims)
    if key not in _cache:
        f = ref.field(name, dims)
        _cache[key] = (f, ref.mesh_ref(f.wsum, f.dsum, f.origin, f.voxel_size, 1.0, f.csum))
    return _cache[key]


def _extract(f, color=True, min_weight=1.0):
    """through from_planes and the entry points themselves, with canaries behind the three outputs -> (vertices, faces, colors) on the host"""
    import fused_tsdf as ft
    w, wb = _padded_plane(f.wsum)
    d, db = _padded_plane(f.dsum)
    c, cb = _padded_plane(f.csum) if color else (None, None)
    before = [b.clone() for b in (wb, db, cb) if b is not None]
    vol = ft.TSDFVolume.from_planes(tuple(float(v) for v in f.origin), float(f.voxel_size), w, d, c)
    lib = ft._lib()
    nodes = f.dims[0] * f.dims[1] * f.dims[2]
    scratch = torch.empty(lib.gsr_tsdf_mesh_scratch_bytes(nodes), dtype=torch.uint8, device=DEV)
    plan = ft.MeshPlan()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    ft._run("gsr_tsdf_mesh_plan", ctypes.byref(vol._grid()), w.data_ptr(), d.data_ptr(), min_weight, scratch.data_ptr(), ctypes.byref(plan), stream)
    V, F = int(plan.V), int(plan.F)
    vert = torch.full((3 * V + GUARD,), CANARY, dtype=torch.float32, device=DEV)
    cols = torch.full((3 * V + GUARD,), CANARY, dtype=torch.float32, device=DEV)
    faces = torch.full((3 * F + GUARD,), -77, dtype=torch.int32, device=DEV)
    # a count that is not the plan's is refused
    for dv, df in ((1, 0), (0, 1), (-1, 0)) if V > 0 else ((1, 0), (0, 1)):
        with pytest.raises(RuntimeError, match="gsr_tsdf_mesh_emit: V .* are not the plan's"):
            ft._run("gsr_tsdf_mesh_emit", ctypes.byref(plan), V + dv, F + df, None, vert.data_ptr(), None, faces.data_ptr(), stream)
    ft._run("gsr_tsdf_mesh_emit", ctypes.byref(plan), V, F, None if c is None else c.data_ptr(), vert.data_ptr(), cols.data_ptr() if color else None,
            faces.data_ptr(), stream)
    torch.cuda.synchronize()
    assert _intact(vert) and _intact(cols) and bool((faces[3 * F:] == -77).all())
    assert all(torch.equal(a, b) for a, b in zip(before, (wb, db, cb)))   # the planes keep their bits
    again = vol.extract_mesh(min_weight=min_weight)                       # the Python surface: the same bits, twice
    third = vol.extract_mesh(min_weight=min_weight)
    for x, y, z in zip(again, third, (vert[:3 * V].view(V, 3), faces[:3 * F].view(F, 3), cols[:3 * V].view(V, 3) if color else None)):
        assert (x is None and y is None and z is None) or (x.shape == z.shape and x.dtype == z.dtype and torch.equal(x, y) and _same(x, z))
    return vert[:3 * V].view(V, 3).cpu().numpy(), faces[:3 * F].view(F, 3).cpu().numpy(), (cols[:3 * V].view(V, 3).cpu().numpy() if color else None)


@pytest.mark.parametrize("dims", ref.MESH_GRIDS)
@pytest.mark.parametrize("name", ("sphere", "plane", "two_spheres", "slab"))
def test_extraction_matches_the_reference_mesh(name, dims):
    f, m = _field(name, dims)
    v, faces, cols = _extract(f)
    assert len(v) == len(m.vertices) and len(faces) == len(m.faces)
    assert np.array_equal(ref.rotate_to_smallest(faces), ref.rotate_to_smallest(m.faces))   # exactly and in order
    if len(v):
        extent = np.maximum(np.abs(m.lower), np.abs(m.upper))
        ev = np.abs(v.astype(np.float64) - m.vertices) / (4 * U * extent)
        cext = np.maximum(np.abs(m.c0), np.abs(m.c1))
        ec = np.abs(cols.astype(np.float64) - m.colors) / (4 * U * cext)
        print(f"{name} {dims}: V = {len(v)}, F = {len(faces)}; largest error / bar: vertices {ev.max():.3f}, colours {ec.max():.3f}")
        assert float(ev.max()) <= 1.0 and float(ec.max()) <= 1.0
    # the topology of the GPU's own faces
    top = ref.topology(faces)
    assert top.manifold
    if name != "slab" and min(dims) >= 8:
        closed = [c for c in top.components if c.closed]
        assert len(closed) == f.spheres and all(c.euler == 2 for c in closed)
    if len(faces) and min(dims) >= 8:   # a smaller grid holds a sphere of less than a voxel: its mesh is the reference's, and no surface
        n = ref.face_normals(v.astype(np.float64), faces)
        dots = (n * f.gradient(v.astype(np.float64)[faces].mean(axis=1))).sum(axis=1)
        assert float(dots.min()) > 0.0
    if name == "slab" and min(dims) >= 8:   # the layer of wsum = 0 opens the sphere: fewer faces than the whole one, and a boundary
        assert 0 < len(faces) < len(_field("sphere", dims)[1].faces) and not any(c.closed for c in top.components)
    # without colour planes: the same vertices and faces, and no colours
    if dims in ((12, 11, 10), (2, 2, 2)):
        v2, f2, c2 = _extract(f, color=False)
        assert c2 is None and v2.tobytes() == v.tobytes() and f2.tobytes() == faces.tobytes()


@pytest.mark.parametrize("name", ("outside", "invalid"))
@pytest.mark.parametrize("dims", ((2, 2, 2), (9, 8, 5)))
def test_a_volume_without_a_surface_gives_the_empty_mesh(name, dims):
    import fused_tsdf as ft
    f = ref.field(name, dims)
    vol = ft.TSDFVolume.from_planes(tuple(float(v) for v in f.origin), float(f.voxel_size), _dev(f.wsum), _dev(f.dsum), _dev(f.csum))
    v, faces, cols = vol.extract_mesh()
    assert v.shape == (0, 3) and faces.shape == (0, 3) and cols.shape == (0, 3) and v.dtype == torch.float32 and faces.dtype == torch.int32
    if name == "outside":   # and all inside: no crossing either
        vol.dsum.neg_()
        assert vol.extract_mesh()[1].shape == (0, 3)
        vol.dsum.zero_()    # exactly 0 counts as outside
        assert vol.extract_mesh()[0].shape == (0, 3)


# ---- extraction without smoothness: every row of the rule, scattered validity, the scan's seams ----
def _fast(key, make, min_weight):
    """a field of torch_tsdf and its array reference (tests/test_tsdf_cpu.py holds that one to the loop reference, bit for bit)"""
    key = ("fast", key, min_weight)
    if key not in _cache:
        f = make()
        _cache[key] = (f, ref.mesh_ref_fast(f.wsum, f.dsum, f.origin, f.voxel_size, min_weight, f.csum))
    return _cache[key]


def _held_to_the_reference(label, m, v, faces, cols):
    """the assertions of test_extraction_matches_the_reference_mesh, the indices' range, and the vertices that lie on a node"""
    assert len(v) == len(m.vertices) and len(faces) == len(m.faces) and len(v) > 0 and len(faces) > 0
    assert int(faces.min()) >= 0 and int(faces.max()) < len(v)
    assert np.array_equal(ref.rotate_to_smallest(faces), ref.rotate_to_smallest(m.faces))   # exactly and in order
    extent = np.maximum(np.abs(m.lower), np.abs(m.upper))
    ev = np.abs(v.astype(np.float64) - m.vertices) / (4 * U * extent)
    cext = np.maximum(np.abs(m.c0), np.abs(m.c1))
    ec = np.abs(cols.astype(np.float64) - m.colors) / (4 * U * cext)
    on_lower, on_upper = m.t == 0, m.t == 1
    print(f"{label}: V = {len(v)}, F = {len(faces)}; largest error / bar: vertices {ev.max():.3f}, colours {ec.max():.3f}; on a node: "
          f"{int(on_lower.sum())} + {int(on_upper.sum())} vertices")
    assert float(ev.max()) <= 1.0 and float(ec.max()) <= 1.0
    # t = 0 or 1: the value at one end is +-0, and the vertex is that node, rounded once
    assert on_lower.any() and on_upper.any()
    assert np.array_equal(v[on_lower], m.lower[on_lower].astype(np.float32)) and np.array_equal(v[on_upper], m.upper[on_upper].astype(np.float32))


@pytest.mark.parametrize("min_weight", (1.0, ref.THRESHOLD))
@pytest.mark.parametrize("dims", ((9, 8, 5), (33, 17, 9)))
def test_extraction_of_noise_with_scattered_invalid_nodes(dims, min_weight):
    """torch_tsdf.noise: values without smoothness, a tenth of them +-0, and at min_weight = 2.0 about half the nodes invalid at random,
    with planted nodes of wsum = 2.0 (valid) and the float32 below it (invalid).  tests/test_tsdf_cpu.py shows what that reaches: all
    6 x 14 rows of the kernel's table (three times and more on the larger grid, at either threshold), cells with emitting and suppressed
    tetrahedra, vertices no face names.  _extract checks the canaries, the planes' bits and extract_mesh(min_weight=) against the entry
    points."""
    f, m = _fast(("noise", dims), lambda: ref.noise(dims), min_weight)
    v, faces, cols = _extract(f, min_weight=min_weight)
    _held_to_the_reference(f"noise {dims} min_weight {min_weight}", m, v, faces, cols)
    if min_weight == 1.0:
        assert ref.topology(faces).manifold
    else:   # a weight of exactly min_weight is valid, the float32 below it is not
        owned = lambda n: int((m.node == n).sum())
        assert all(owned(n) > 0 for n in f.planted_valid[:, 0]) and not any(owned(n) for n in f.planted_invalid[:, 0])


def test_extraction_across_the_wave_seam_of_the_plan_scan():
    """noise over (65, 64, 17): 277 count workgroups, each with vertices, so scan threads 0..69 hold data and the prefix over the scan's
    wave totals (`k < w` in gsr_tsdf_block_scan<16>) moves workgroups 256..276 by the whole of wave 0.  Reaches: the wave seam 63 | 64."""
    f, m = _fast("wave seam", lambda: ref.noise(ref.WAVE_SEAM_DIMS), 1.0)
    v, faces, cols = _extract(f)
    _held_to_the_reference(f"noise {ref.WAVE_SEAM_DIMS}", m, v, faces, cols)


def test_extraction_across_the_chunk_seam_of_the_plan_scan():
    """torch_tsdf.seam_field, (128, 128, 66): 4 224 count workgroups, more than the 4 096 the scan takes in one trip.  Noise sits in
    thin bands placed by n // 256 and the constant outside value everywhere else, so that (seam_layout asserts it on the reference
    before anything runs) vertices and triangles lie in workgroups 255 | 256 and 511 | 512 (scan threads 63 | 64 and 127 | 128: two wave
    seams), 1 023 | 1 024, 4 095 | 4 096 (the second trip: its bases are the 64-bit carry plus a prefix that starts again at 0) and in the
    last workgroup with a whole cell, 4 159, with 384 empty workgroups in between where the prefix must stay flat.  Every vertex id and
    face index behind a seam is wrong by a whole wave's or trip's total if the seam is: the faces are compared exactly and in order.
    Not reached: the truncation of the bases to 32 bits ("emit is refused where they do not fit"), which needs more than 2^31
    vertices."""
    import time
    f, m = _fast("seam", ref.seam_field, 1.0)
    per_group_v, _ = ref.seam_layout(m)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v, faces, cols = _extract(f)
    wall = time.perf_counter() - t0
    _held_to_the_reference(f"seam volume {ref.SEAM_DIMS} ({len(per_group_v)} workgroups, _extract took {1e3 * wall:.0f} ms)", m, v, faces, cols)


# ---- end to end ----
def test_sphere_scene_fuses_to_within_a_voxel():
    import fused_tsdf as ft
    S = ref.SPHERE
    origin, vs, rec, depth = ref.sphere_scene()
    vol = ft.TSDFVolume(tuple(float(v) for v in origin), float(vs), S.dims, sdf_trunc=S.trunc_voxels * float(vs), color=False, device=DEV)
    vol.integrate(_dev(depth), _dev(rec))
    v, faces, cols = vol.extract_mesh()
    assert cols is None and len(faces) > 3000
    vn = v.double().cpu().numpy()
    dist = np.abs(np.linalg.norm(vn, axis=1) - S.radius) / float(vs)
    print(f"sphere scene: V = {len(v)}, F = {len(faces)}, largest distance {dist.max():.3f} voxel_size, mean {dist.mean():.3f}")
    assert float(dist.max()) < 1.0
    assert ref.topology(faces.cpu().numpy()).manifold and int(faces.min()) >= 0 and int(faces.max()) < len(v)
    n = ref.face_normals(vn, faces.cpu().numpy())
    outward = (n * vn[faces.cpu().numpy()].mean(axis=1)).sum(axis=1)
    assert float((outward > 0).mean()) > 0.99   # the faces look out of the sphere, towards the cameras


def test_median_depth_of_the_renderer_fuses_into_a_mesh():
    """plumbing on the real renderer: four ring cameras at 64 x 48 around a small cloud, median depth and colour into 24^3"""
    import fused_tsdf as ft
    import gaussian_renderer
    import gsr_model
    import gsr_scene
    scene = gsr_scene.make_scene(400, -2.0, sh_degree=0, seed=11)
    pc = gsr_model.GaussianParams.from_activated(scene.means3D, scene.shs, scene.scales, scene.rotations, scene.opacities, device=DEV, active_sh_degree=0)
    pipe = gsr_model.pipeline_params()
    bg = scene.bg.to(DEV)
    centre = scene.means3D.mean(dim=0)
    spread = float((scene.means3D - centre).abs().max())
    cams = [gsr_scene.ring_camera(64, 48, k, 4) for k in range(4)]
    half = 1.2 * spread
    origin = tuple(float(c) - half for c in centre)

    def fuse():
        vol = ft.TSDFVolume(origin, 2.0 * half / 23, (24, 24, 24), device=DEV)
        hit = 0
        for cam in cams:
            camd = cam._replace(world_view_transform=cam.world_view_transform.to(DEV), full_proj_transform=cam.full_proj_transform.to(DEV),
                                camera_center=cam.camera_center.to(DEV))
            with torch.no_grad():
                out = gaussian_renderer.render(camd, pc, pipe, bg, depth_alpha="depth", median_depth=True)
            alpha = out["alpha"]
            hit += int((alpha > 0.5).sum())
            vol.integrate(out["median_depth"], [cam], color=out["render"].clamp(0, 1), weight=(alpha > 0.5).float())
        return vol, vol.extract_mesh(), hit

    vol, (v, faces, cols), hit = fuse()
    assert hit > 0 and float(vol.wsum.max()) >= 1.0
    assert len(v) > 0 and len(faces) > 0 and cols.shape == v.shape
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(cols).all()) and float(cols.min()) >= 0.0 and float(cols.max()) <= 1.0 + 1e-6
    lo = torch.tensor(origin, device=DEV)
    assert bool((v >= lo - 1e-5).all()) and bool((v <= lo + 2.0 * half + 1e-5).all())   # inside the volume
    assert int(faces.min()) >= 0 and int(faces.max()) < len(v)
    _, (v2, f2, c2), _ = fuse()
    assert _same(v, v2) and torch.equal(faces, f2) and _same(cols, c2)                   # identical on a second run
