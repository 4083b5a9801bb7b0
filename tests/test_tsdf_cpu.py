"""CPU: TSDF fusion and marching tetrahedra (include/gsr_tsdf.h, fused_tsdf.py, gsr_ply.write_mesh_ply) without a device.  The header
compiles as C99 and as C++17 beside gsr.h and when included twice; every function it declares is exported; the ctypes records are the
header's; the scratch function returns 0 for invalid sizes and stays within 8 bytes a node; every entry point validates its arguments
before any device work; the Python surface refuses before the kernel library is loaded; a mesh file round-trips bit for bit.  The
float64 reference of tests/torch_tsdf.py, built from the generic rule and a cross product, gives closed, consistently oriented surfaces
of the right Euler characteristic whose vertices lie on their grid edges.  The integration scenes of the GPU test have at most 1 %
ambiguous nodes, and in each of them (but the grid of one node) pairs are skipped, cut at -sdf_trunc and clamped to 1.
The end-to-end scene (six cameras on the axes, 3 units from a sphere of radius 0.5, 64 x 64 pixels at focal 100, a 24^3 grid of voxel
0.0696, sdf_trunc of 3 voxels), fused and meshed by the reference: every vertex within 0.860 voxel_size of the sphere, 0.156 in the
mean (with the default truncation of 4 voxels it is 1.09: the projective distance at grazing rays).
The array form of the reference (mesh_ref_fast, for volumes of a million nodes) equals the loop form byte for byte on every field of
the GPU's extraction tests; the noise field reaches all 6 x 14 (tetrahedron, case) rows, all seven edge kinds, t = 0 and t = 1, and at
min_weight = 2.0 suppressed tetrahedra beside emitting ones, unnamed vertices and the planted weights at the threshold; the seam volume
has counts on both sides of every seam of the plan's scan.  Nothing here touches a device."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import torch_tsdf as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsr_tsdf.h")
LIB = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "libgsr_hip.so")
INVALID = -1   # GSR_ERR_INVALID_ARGUMENT
NAMES = ["gsr_tsdf_integrate", "gsr_tsdf_mesh_emit", "gsr_tsdf_mesh_plan", "gsr_tsdf_mesh_scratch_bytes"]
_meshes = {}


def _lib():
    import fused_tsdf as ft
    if not os.path.exists(LIB):
        __graft_entry__.build()
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L = ctypes.CDLL(LIB)
    L.gsr_last_error.restype = ctypes.c_char_p
    L.gsr_tsdf_integrate.argtypes = [ctypes.POINTER(ft.Grid), vp, vp, vp, i, vp, vp, i, i, vp, vp, vp, f, f, vp]
    L.gsr_tsdf_mesh_scratch_bytes.restype = ctypes.c_size_t
    L.gsr_tsdf_mesh_scratch_bytes.argtypes = [ctypes.c_longlong]
    L.gsr_tsdf_mesh_plan.argtypes = [ctypes.POINTER(ft.Grid), vp, vp, f, vp, ctypes.POINTER(ft.MeshPlan), vp]
    L.gsr_tsdf_mesh_emit.argtypes = [ctypes.POINTER(ft.MeshPlan), ctypes.c_longlong, ctypes.c_longlong, vp, vp, vp, vp, vp]
    return L


def _mesh(name, dims):
    """the field and its reference mesh, computed once"""
    if (name, dims) not in _meshes:
        f = ref.field(name, dims)
        _meshes[(name, dims)] = (f, ref.mesh_ref(f.wsum, f.dsum, f.origin, f.voxel_size, 1.0, f.csum))
    return _meshes[(name, dims)]


# ---- the header and the library ----
@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_alongside_the_core_abi(tmp_path, compiler, std, ext):
    src = tmp_path / f"includer.{ext}"
    src.write_text('#include "gsr.h"\n#include "gsr_tsdf.h"\n#include "gsr_tsdf.h"\n'
                   "int gsr_tsdf_includer(void) { return (int)(sizeof(&gsr_tsdf_integrate) + sizeof(&gsr_tsdf_mesh_plan) + sizeof(&gsr_tsdf_mesh_emit) + "
                   "sizeof(&gsr_tsdf_mesh_scratch_bytes) + sizeof(gsr_tsdf_grid) + sizeof(gsr_tsdf_mesh_plan_t) + sizeof(&gsr_adam_step)) + "
                   "GSR_TSDF_THREADS; }\n"
                   "typedef char gsr_tsdf_brick_is_a_workgroup[GSR_TSDF_BRICK_X * GSR_TSDF_BRICK_Y * GSR_TSDF_BRICK_Z == GSR_TSDF_THREADS ? 1 : -1];\n")
    r = subprocess.run([compiler, std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_every_declared_symbol_is_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr)))
    assert names == NAMES, names
    L = _lib()
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/gsr_tsdf.h but not exported"


def test_record_layout_and_constants_match_the_header(tmp_path):
    import fused_tsdf as ft
    hdr = open(HDR).read()
    defines = dict(re.findall(r"#define (GSR_TSDF_[A-Z_]+) (0x[0-9a-f]+|[0-9]+)", hdr))
    assert int(defines["GSR_TSDF_THREADS"]) == ft.THREADS
    assert int(defines["GSR_TSDF_PLAN_MAGIC"], 16) == ft.PLAN_MAGIC
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsr_tsdf.h"\nint main(void) { printf("%d %d %d %d %d %d %d\\n", (int)sizeof(gsr_tsdf_grid), '
                   "(int)offsetof(gsr_tsdf_grid, origin), (int)offsetof(gsr_tsdf_grid, voxel_size), (int)sizeof(gsr_tsdf_mesh_plan_t), "
                   "(int)offsetof(gsr_tsdf_mesh_plan_t, grid), (int)offsetof(gsr_tsdf_mesh_plan_t, wsum), (int)offsetof(gsr_tsdf_mesh_plan_t, min_weight)); "
                   "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got == [ctypes.sizeof(ft.Grid), ft.Grid.origin.offset, ft.Grid.voxel_size.offset, ctypes.sizeof(ft.MeshPlan), ft.MeshPlan.grid.offset,
                   ft.MeshPlan.wsum.offset, ft.MeshPlan.min_weight.offset]


def test_scratch_size_is_zero_for_invalid_sizes_and_at_most_eight_bytes_a_node():
    L = _lib()
    for nodes in (0, -1, 1, 7, 1 << 31, 1 << 40):
        assert L.gsr_tsdf_mesh_scratch_bytes(nodes) == 0, nodes
    prev = 0
    for nodes in (8, 12, 255, 256, 257, 5049, 1 << 24, 512 ** 3, (1 << 31) - 1):
        b = L.gsr_tsdf_mesh_scratch_bytes(nodes)
        assert 5 * nodes < b <= 8 * nodes and b >= prev, (nodes, b)
        prev = b


def test_entry_points_validate_before_any_device_work():
    import fused_tsdf as ft
    L = _lib()
    one = 4096   # a non-NULL address that must never be dereferenced
    nan, inf = float("nan"), float("inf")

    def grid(nx=8, ny=8, nz=8, origin=(0.0, 0.0, 0.0), vs=0.1):
        return ft.Grid(nx, ny, nz, (ctypes.c_float * 3)(*origin), vs)

    cams = (ft_camera() * 2)()
    for c in cams:
        c.W, c.H = 64.0, 48.0

    def integrate(g=None, wsum=one, dsum=one, csum=one, C=2, cameras=one, host=None, H=48, W=64, depth=one, color=one, weight=one, trunc=0.4,
                  dtrunc=inf):
        gp = ctypes.byref(grid() if g is None else g) if g != "null" else None
        return L.gsr_tsdf_integrate(gp, wsum, dsum, csum, C, cameras, host, H, W, depth, color, weight, trunc, dtrunc, None)

    wrong_w, wrong_h = (ft_camera() * 2)(), (ft_camera() * 2)()
    for a, b in zip(wrong_w, wrong_h):
        a.W, a.H, b.W, b.H = 64.0, 48.0, 64.0, 48.0
    wrong_w[1].W, wrong_h[0].H = 63.0, 49.0
    bad = [dict(g="null"), dict(g=grid(nx=0)), dict(g=grid(ny=0)), dict(g=grid(nz=-1)), dict(g=grid(2048, 2048, 512)), dict(g=grid(65536, 65536, 1)),
           dict(g=grid(vs=0.0)), dict(g=grid(vs=-1.0)), dict(g=grid(vs=nan)), dict(g=grid(vs=inf)), dict(g=grid(origin=(0.0, nan, 0.0))),
           dict(g=grid(origin=(inf, 0.0, 0.0))), dict(wsum=None), dict(dsum=None), dict(cameras=None), dict(depth=None), dict(csum=None),
           dict(C=0), dict(C=-2), dict(H=0), dict(W=0), dict(W=-5), dict(W=(1 << 24) + 1), dict(H=1 << 16, W=1 << 16), dict(trunc=0.0), dict(trunc=-1.0),
           dict(trunc=nan), dict(trunc=inf), dict(dtrunc=0.0), dict(dtrunc=-1.0), dict(dtrunc=nan),
           dict(host=ctypes.addressof(wrong_w)), dict(host=ctypes.addressof(wrong_h)), dict(host=ctypes.addressof(cams), W=63), dict(host=ctypes.addressof(cams), H=47)]
    for kw in bad:
        assert integrate(**kw) == INVALID, kw
        assert L.gsr_last_error().startswith(b"gsr_tsdf_integrate:"), (kw, L.gsr_last_error())

    def plan(g=None, wsum=one, dsum=one, min_weight=1.0, scratch=one, out="own"):
        gp = ctypes.byref(grid() if g is None else g) if g != "null" else None
        return L.gsr_tsdf_mesh_plan(gp, wsum, dsum, min_weight, scratch, ctypes.byref(ft.MeshPlan()) if out == "own" else out, None)

    for kw in (dict(g="null"), dict(g=grid(nx=1)), dict(g=grid(ny=1)), dict(g=grid(nz=1)), dict(g=grid(nz=0)), dict(g=grid(2048, 2048, 512)),
               dict(g=grid(vs=0.0)), dict(g=grid(vs=nan)), dict(g=grid(origin=(0.0, 0.0, inf))), dict(wsum=None), dict(dsum=None), dict(scratch=None),
               dict(scratch=4100), dict(out=None), dict(min_weight=0.0), dict(min_weight=-1.0), dict(min_weight=nan), dict(min_weight=inf)):
        assert plan(**kw) == INVALID, kw
        assert L.gsr_last_error().startswith(b"gsr_tsdf_mesh_plan:"), (kw, L.gsr_last_error())

    def emit(V=10, F=12, change=None, csum=one, vertices=one, colors=one, faces=one, null=False):
        p = ft.MeshPlan(V=10, F=12, grid=grid(), wsum=one, dsum=one, scratch=one, min_weight=1.0, magic=ft.PLAN_MAGIC)
        if change:
            change(p)
        return L.gsr_tsdf_mesh_emit(None if null else ctypes.byref(p), V, F, csum, vertices, colors, faces, None)

    def setter(name, value):
        return lambda p: setattr(p, name, value)

    for kw in (dict(null=True), dict(change=setter("magic", 0)), dict(change=setter("grid", grid(nx=1))), dict(change=setter("wsum", None)),
               dict(change=setter("scratch", None)), dict(V=11), dict(F=11), dict(V=0, F=0), dict(V=-1), dict(F=-1), dict(V=1 << 31), dict(F=1 << 40),
               dict(change=setter("V", 1 << 31), V=1 << 31), dict(change=setter("F", 1 << 33), F=1 << 33), dict(csum=None), dict(vertices=None),
               dict(faces=None)):
        assert emit(**kw) == INVALID, kw
        assert L.gsr_last_error().startswith(b"gsr_tsdf_mesh_emit:"), (kw, L.gsr_last_error())


def ft_camera():
    import fused_filter3d as ff
    return ff.FilterCamera


def _dress(t):
    """a CPU tensor whose `device` attribute says cuda:0: for the checks that lie behind the device check and touch no device"""
    cuda = torch.device("cuda", 0)

    class T(torch.Tensor):
        @property
        def device(self):
            return cuda
    return t.as_subclass(T)


def test_python_surface_refuses_before_the_library_loads():
    import fused_filter3d as ff
    import fused_tsdf as ft
    import torch_filter3d
    from diff_gaussian_rasterization import _C, CameraModel
    loaded = _C._lib
    _C._lib = None
    try:
        ok = dict(origin=(0.0, 0.0, 0.0), voxel_size=0.1, dims=(4, 4, 4))
        for kw, exc in ((dict(device="cpu"), RuntimeError), (dict(voxel_size=0.0), ValueError), (dict(voxel_size=float("nan")), ValueError),
                        (dict(voxel_size="1"), TypeError), (dict(dims=(4, 4)), ValueError), (dict(dims=(4, 0, 4)), ValueError),
                        (dict(dims=(4, 4.0, 4)), ValueError), (dict(dims=(2048, 2048, 512)), ValueError), (dict(origin=(0.0, 0.0)), ValueError),
                        (dict(origin=(0.0, float("inf"), 0.0)), ValueError), (dict(sdf_trunc=0.0), ValueError), (dict(sdf_trunc=float("inf")), ValueError),
                        (dict(depth_trunc=0.0), ValueError), (dict(depth_trunc=float("nan")), ValueError), (dict(color=1), TypeError)):
            with pytest.raises(exc):
                ft.TSDFVolume(**{**ok, "device": "cpu", **kw})
        w = torch.ones(4, 5, 6)
        with pytest.raises(RuntimeError, match="no CPU path"):
            ft.TSDFVolume.from_planes((0.0, 0.0, 0.0), 0.1, w, w.clone())
        with pytest.raises(RuntimeError, match="float32"):
            ft.TSDFVolume.from_planes((0.0, 0.0, 0.0), 0.1, w.double(), w.clone())
        with pytest.raises(RuntimeError, match="contiguous"):
            ft.TSDFVolume.from_planes((0.0, 0.0, 0.0), 0.1, w.transpose(0, 1), w.clone())
        for a, b, c in ((w, w[:3], None), (w[0], w[0], None), (w, w.clone(), torch.ones(2, 4, 5, 6)), (w, w.clone(), w.clone())):
            with pytest.raises(RuntimeError, match=r"\(NZ, NY, NX\)"):
                ft.TSDFVolume.from_planes((0.0, 0.0, 0.0), 0.1, a, b, c)
        with pytest.raises(TypeError):
            ft.TSDFVolume.from_planes((0.0, 0.0, 0.0), 0.1, [1.0], w)

        vol = ft.TSDFVolume.from_planes((0.0, 0.0, 0.0), 0.1, _dress(w), _dress(w.clone()), _dress(torch.ones(3, 4, 5, 6)))
        assert vol.dims == (6, 5, 4) and vol.sdf_trunc == pytest.approx(0.4) and vol.depth_trunc == math.inf
        cams = torch_filter3d.ring_cameras(2)   # 64 x 48
        rec = ff.pack_cameras(cams, "cpu")
        depth = torch.ones(2, 48, 64)
        with pytest.raises(RuntimeError, match="no CPU path"):
            vol.integrate(depth, cams)
        with pytest.raises(RuntimeError, match="no CPU path"):
            vol.integrate(_dress(depth), rec)
        with pytest.raises(RuntimeError, match="float32"):
            vol.integrate(depth.double(), cams)
        for bad in (depth[:1], depth[0], torch.ones(2, 2, 48, 64), torch.ones(48)):
            with pytest.raises(RuntimeError, match="depth must be"):
                vol.integrate(bad, cams)
        for bad in (rec[:, :19], rec[:0], rec.double(), rec[0]):
            with pytest.raises(RuntimeError, match="cameras must be"):
                vol.integrate(depth, bad)
        for bad in ([], None, 3):
            with pytest.raises(TypeError, match="cameras must be"):
                vol.integrate(depth, bad)
        with pytest.raises(TypeError):
            vol.integrate([[1.0]], cams)
        with pytest.raises(RuntimeError, match="color must be"):
            vol.integrate(depth, cams, color=torch.ones(2, 3, 48, 63))
        with pytest.raises(RuntimeError, match="weight must have"):
            vol.integrate(depth, cams, weight=torch.ones(2, 48, 63))
        with pytest.raises(RuntimeError, match="float32"):
            vol.integrate(depth, cams, weight=torch.ones(2, 48, 64, dtype=torch.float64))
        with pytest.raises(RuntimeError, match=r"camera 0 is 64 x 48, the depth maps are 32 x 48"):
            vol.integrate(_dress(torch.ones(2, 48, 32)), cams)
        plain = ft.TSDFVolume.from_planes((0.0, 0.0, 0.0), 0.1, _dress(w), _dress(w.clone()))
        with pytest.raises(RuntimeError, match="color=True"):
            plain.integrate(depth, cams, color=torch.ones(2, 3, 48, 64))
        fish = torch_filter3d.ring_cameras(2)
        fish[1].camera_model = CameraModel("fisheye", 60.0, 60.0, 32.0, 24.0)
        with pytest.raises(NotImplementedError, match="fisheye"):
            vol.integrate(depth, fish)
        for mw in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="min_weight"):
                vol.extract_mesh(min_weight=mw)
        with pytest.raises(TypeError, match="min_weight"):
            vol.extract_mesh(min_weight="1")
        flat = ft.TSDFVolume.from_planes((0.0, 0.0, 0.0), 0.1, _dress(torch.ones(1, 5, 6)), _dress(torch.ones(1, 5, 6)))
        with pytest.raises(ValueError, match="at least 2 nodes"):
            flat.extract_mesh()
        with pytest.raises(RuntimeError, match="no CPU path"):
            _cpu_volume(ft, w).extract_mesh()
        assert _C._lib is None, "a refusal loaded the kernel library"
    finally:
        _C._lib = loaded


def _cpu_volume(ft, w):
    """a volume object around CPU planes, as no constructor would make it"""
    vol = ft.TSDFVolume.__new__(ft.TSDFVolume)
    vol._setup((0.0, 0.0, 0.0), 0.1, (6, 5, 4), None, math.inf)
    vol.wsum, vol.dsum, vol.csum = w, w.clone(), None
    return vol


# ---- mesh files ----
@pytest.mark.parametrize("with_colors", (False, True))
def test_mesh_ply_round_trips_bit_for_bit(tmp_path, with_colors):
    import gsr_ply
    _, m = _mesh("sphere", (12, 11, 10))
    v = m.vertices.astype(np.float32)
    f = m.faces.astype(np.int32)
    c = np.random.default_rng(3).integers(0, 256, (len(v), 3)).astype(np.uint8) if with_colors else None
    path = str(tmp_path / "sub" / "mesh.ply")
    gsr_ply.write_mesh_ply(path, torch.from_numpy(v), torch.from_numpy(f), c)
    v2, f2, c2 = gsr_ply.read_mesh_ply(path)
    assert v2.dtype == np.float32 and f2.dtype == np.int32 and v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()
    assert (c2 is None) if c is None else (c2.dtype == np.uint8 and c2.tobytes() == c.tobytes())
    raw = open(path, "rb").read(400).split(b"end_header\n")[0]
    head = raw.decode().split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    assert "property list uchar int vertex_indices" in head and f"element face {len(f)}" in head
    assert ("property uchar red" in head) == with_colors
    assert os.path.getsize(path) == len(raw) + len("end_header\n") + len(v) * (15 if with_colors else 12) + len(f) * 13
    # the point-cloud reader still reads the vertex element of such a file, and still refuses a list
    cloud = gsr_ply.read_ply(path)
    assert np.array_equal(cloud["x"], v[:, 0]) and np.array_equal(cloud["z"], v[:, 2]) and (("red" in cloud) == with_colors)
    with pytest.raises(ValueError, match="list properties"):
        gsr_ply.read_ply(path, element="face")
    # floating-point colours are scaled and rounded
    if with_colors:
        gsr_ply.write_mesh_ply(path, v, f, c.astype(np.float32) / 255.0)
        assert gsr_ply.read_mesh_ply(path)[2].tobytes() == c.tobytes()
    with pytest.raises(ValueError, match="outside"):
        gsr_ply.write_mesh_ply(path, v[:5], f)


def test_an_empty_mesh_round_trips(tmp_path):
    import gsr_ply
    path = str(tmp_path / "empty.ply")
    for colors in (None, np.zeros((0, 3), np.uint8)):
        gsr_ply.write_mesh_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), colors)
        v, f, c = gsr_ply.read_mesh_ply(path)
        assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == np.float32 and f.dtype == np.int32
        assert (c is None) if colors is None else c.shape == (0, 3)
        assert len(gsr_ply.read_ply(path)["x"]) == 0


# ---- the reference mesh ----
@pytest.mark.parametrize("dims", ((12, 11, 10), (17, 9, 8)))
@pytest.mark.parametrize("name", ("sphere", "plane", "two_spheres"))
def test_reference_mesh_is_closed_oriented_and_on_its_edges(name, dims):
    f, m = _mesh(name, dims)
    assert len(m.faces) > 100 and int(m.faces.min()) == 0 and int(m.faces.max()) == len(m.vertices) - 1
    top = ref.topology(m.faces)
    assert top.manifold                                                   # no directed edge twice: neighbours agree on the orientation
    closed = [c for c in top.components if c.closed]
    assert len(closed) == f.spheres and len(top.components) == max(f.spheres, 1)
    assert all(c.euler == 2 for c in closed)
    if name == "plane":                                                   # open at the boundary of the grid only: a disc
        assert top.components[0].euler == 1
    n = ref.face_normals(m.vertices, m.faces)
    dots = (n * f.gradient(m.vertices[m.faces].mean(axis=1))).sum(axis=1)
    assert float(dots.min()) > 0.0
    # every vertex lies on its grid edge, where the interpolated field is 0
    assert bool(((m.t >= 0) & (m.t <= 1)).all())
    assert float(np.abs(m.vertices - (m.lower + m.t[:, None] * (m.upper - m.lower))).max()) <= 1e-12
    assert float(np.abs((1 - m.t) * m.v0 + m.t * m.v1).max()) <= 1e-12
    assert bool((((m.upper - m.lower) / float(f.voxel_size)).round(6).max(axis=1) == 1.0).all())
    # and within the linear interpolation's error of the analytic surface
    assert float(np.abs(f.value(m.vertices)).max()) < 0.25 * float(f.voxel_size)
    # the order of the contract: vertices ascend in (node, kind) -- the lower node's position is sorted z, y, x
    key = np.round((m.lower - f.origin.astype(np.float64)) / float(f.voxel_size)).astype(np.int64)
    lin = key[:, 0] + dims[0] * (key[:, 1] + dims[1] * key[:, 2])
    assert bool((np.diff(lin) >= 0).all())
    print(f"{name} {dims}: V = {len(m.vertices)}, F = {len(m.faces)}, smallest normal . gradient {dots.min():.2e}")


def test_generic_rule_gives_one_or_two_triangles():
    corners = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)]
    for m in range(16):
        inside = [bool(m >> l & 1) for l in range(4)]
        tris = ref.tet_triangles(corners, inside)
        assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[sum(inside)]
        for t in tris:
            assert all(inside[a] != inside[b] for a, b in t) and len(set(t)) == 3


# ---- the array reference, which serves the grids the loops cannot ----
FIELDS_OF_A_MESH = ("vertices", "lower", "upper", "v0", "v1", "t", "faces", "c0", "c1", "colors", "node", "kind", "cell", "tet", "case")


def _pinned(f, loop, min_weight):
    """mesh_ref_fast of the field, after holding every field of it to the bits of `loop`"""
    fast = ref.mesh_ref_fast(f.wsum, f.dsum, f.origin, f.voxel_size, min_weight, f.csum)
    assert len(fast.vertices) == len(loop.vertices) and len(fast.faces) == len(loop.faces)
    assert np.array_equal(fast.faces, loop.faces)                         # as arrays, in order
    for name in FIELDS_OF_A_MESH:
        a, b = getattr(fast, name), getattr(loop, name)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    return fast


@pytest.mark.parametrize("dims", ref.MESH_GRIDS)
@pytest.mark.parametrize("name", ("sphere", "plane", "two_spheres", "slab"))
def test_array_reference_is_the_loop_reference_bit_for_bit(name, dims):
    """Every pair of the GPU's extraction test.  No bound: mesh_ref_fast applies mesh_ref's formulas to the same doubles in the same
    order (t = v0 / (v0 - v1), lo + t (up - lo), c0 + t (c1 - c0), the positions as origin + index * voxel_size), so float64 fields are
    compared as bytes, and so are the faces and the (node, kind), (cell, tetrahedron, case) that say where each row came from."""
    f, m = _mesh(name, dims)
    _pinned(f, m, 1.0)


def _noise(dims, min_weight):
    """the noise field, its loop reference and its census, computed once"""
    key = ("noise", dims, min_weight)
    if key not in _meshes:
        f = ref.noise(dims)
        _meshes[key] = (f, ref.mesh_ref(f.wsum, f.dsum, f.origin, f.voxel_size, min_weight, f.csum), ref.tet_census(f.wsum, min_weight, f.dsum))
    return _meshes[key]


@pytest.mark.parametrize("min_weight", (1.0, ref.THRESHOLD))
@pytest.mark.parametrize("dims", ((9, 8, 5), (33, 17, 9)))
def test_noise_field_reaches_every_row_of_the_rule_and_scattered_validity(dims, min_weight):
    """Conditions on the inputs of the GPU test, taken from the loop reference (and the array reference pinned to it on the way): all
    6 x 14 (tetrahedron, case) pairs among the tetrahedra with four valid corners -- once on the small grid at min_weight 1, three times
    on the larger at both thresholds (at 2.0 the small grid has some fifty whole tetrahedra: no claim) -- all seven edge kinds, vertices
    at t = 0 and t = 1 exactly, and at the threshold: cells where one tetrahedron emits and another with a crossed edge is suppressed by
    an invalid corner, vertices that no face names, and the planted nodes: wsum = 2.0 owns a vertex on its +x edge, the float32 below
    2.0 owns none."""
    f, m, cen = _noise(dims, min_weight)
    _pinned(f, m, min_weight)
    counts = np.zeros((6, 16), np.int64)
    for T in range(6):
        counts[T] = np.bincount(cen.case[cen.whole[:, T], T], minlength=16)
    least = int(counts[:, 1:15].min())
    emitting = cen.whole & (cen.case > 0) & (cen.case < 15)
    suppressed = ~cen.whole & cen.crossed
    both = int((emitting.any(axis=1) & suppressed.any(axis=1)).sum())
    unnamed = len(m.vertices) - len(np.unique(m.faces))
    print(f"noise {dims} min_weight {min_weight}: V = {len(m.vertices)}, F = {len(m.faces)}, whole tetrahedra {int(cen.whole.sum())}, least (T, case) count "
          f"{least}, t = 0: {int((m.t == 0).sum())}, t = 1: {int((m.t == 1).sum())}, cells emitting and suppressed {both}, unnamed vertices {unnamed}")
    # the faces come from exactly the emitting tetrahedra, in their order
    per_case = np.array([0] + [2 if bin(c).count("1") == 2 else 1 for c in range(1, 15)] + [0])
    assert np.array_equal(np.bincount(m.tet * 16 + m.case, minlength=96).reshape(6, 16), counts * per_case[None])
    if dims == (9, 8, 5):
        assert min_weight != 1.0 or least >= 1
    else:
        assert least >= 3
    assert sorted(set(m.kind.tolist())) == list(range(7))
    assert bool((m.t == 0).any()) and bool((m.t == 1).any()) and bool(((m.t >= 0) & (m.t <= 1)).all())
    assert int((f.dsum == 0).sum()) >= f.dsum.size // 20 and bool(np.signbit(f.dsum[f.dsum == 0]).any()) and not bool(np.signbit(f.dsum[f.dsum == 0]).all())
    w = f.wsum.reshape(-1)
    below = np.nextafter(np.float32(ref.THRESHOLD), np.float32(0.0))
    assert bool((w[f.planted_valid[:, 0]] == np.float32(ref.THRESHOLD)).all()) and bool((w[f.planted_invalid[:, 0]] == below).all())
    assert len(f.planted_valid) >= 4 and len(f.planted_invalid) >= 4 and bool((w[np.concatenate([f.planted_valid, f.planted_invalid])[:, 1]] >= ref.THRESHOLD).all())
    owns = lambda n: int(((m.node == n) & (m.kind == 0)).sum())
    assert all(owns(n) == 1 for n in f.planted_valid[:, 0])
    if min_weight == 1.0:
        assert ref.topology(m.faces).manifold and both == 0 and unnamed == 0 and all(owns(n) == 1 for n in f.planted_invalid[:, 0])
    else:
        assert both > 0 and unnamed > 0 and not any(int((m.node == n).sum()) for n in f.planted_invalid[:, 0])


def _seam():
    if "seam" not in _meshes:
        f = ref.seam_field()
        _meshes["seam"] = (f, ref.mesh_ref_fast(f.wsum, f.dsum, f.origin, f.voxel_size, 1.0, f.csum))
    return _meshes["seam"]


def test_seam_volume_puts_counts_on_both_sides_of_every_seam_of_the_scan():
    """The layout the GPU test relies on (torch_tsdf.seam_layout asserts it; the GPU test calls the same function): more than 4 096
    count workgroups; vertices and triangles in workgroups 255 | 256 and 511 | 512 (scan threads 63 | 64, 127 | 128), 4 095 | 4 096 (the
    second trip of the chunk loop) and in the last workgroup that holds a whole cell; triangles beyond 4 096; 64 or more consecutive
    workgroups without any; V and F below 400 000.  And where the noise is not, nothing: every count lies in a noisy layer or the one
    below it."""
    f, m = _seam()
    v, t = ref.seam_layout(m)
    layers = np.flatnonzero((v + t).reshape(ref.SEAM_DIMS[2], -1).sum(axis=1))
    assert set(layers) <= set(ref.SEAM_LAYERS) | {k - 1 for k in ref.SEAM_LAYERS}
    assert v[1023] > 0 and v[1024] > 0 and t[1023] > 0 and t[1024] > 0   # and the seam of waves 3 | 4
    print(f"seam volume {ref.SEAM_DIMS}: V = {len(m.vertices)}, F = {len(m.faces)}, {len(v)} workgroups, {int((v > 0).sum())} with vertices, "
          f"{int((t > 0).sum())} with triangles, the last with a cell {int(np.flatnonzero(t)[-1])}")
    # the wave-seam volume: dense counts on either side of workgroups 255 | 256
    g = ref.noise(ref.WAVE_SEAM_DIMS)
    v, t = ref.workgroup_counts(ref.mesh_ref_fast(g.wsum, g.dsum, g.origin, g.voxel_size, 1.0), ref.WAVE_SEAM_DIMS)
    assert len(v) > 256 and bool((v > 0).all()) and bool((t[:260] > 0).all())


# ---- the scenes of the GPU tests ----
@pytest.mark.parametrize("image", ref.IMAGES)
@pytest.mark.parametrize("C", ref.CAMERAS)
@pytest.mark.parametrize("dims", ref.GRIDS)
def test_ambiguous_nodes_of_the_gpu_scenes_stay_under_the_cap(dims, C, image):
    """The GPU test skips the nodes where a decision lies inside the fp32 error of its own inputs: at most 1 % of them.  In every scene
    pairs are skipped, cut at -sdf_trunc and clamped to 1; the grid of one node has a single pair per camera and is exempt."""
    s = ref.integration_scene(dims, C, image)
    r = ref.integrate_ref(dims, s.origin, s.voxel_size, s.rec, s.depth, s.color, s.weight, wsum0=s.wsum0, dsum0=s.dsum0, csum0=s.csum0)
    nodes = dims[0] * dims[1] * dims[2]
    print(f"{dims} C = {C} {image}: {int(r.ambiguous.sum())} ambiguous of {nodes}, {int(r.touched.sum())} touched; pairs skipped {r.skipped}, cut {r.cut}, "
          f"clamped {r.clamped}")
    assert int(r.ambiguous.sum()) <= nodes // 100
    assert r.skipped + r.cut <= nodes * C
    if nodes > 1:
        assert r.skipped > 0 and r.cut > 0 and r.clamped > 0
        assert bool(r.touched.any()) and not bool(r.touched.all())
    for name in ("zeros", "nan", "inf", "beyond", "negative"):
        d = s.depth
        hit = {"zeros": d == 0, "nan": np.isnan(d), "inf": np.isinf(d), "beyond": d > ref.DEPTH_TRUNC, "negative": d < 0}[name]
        assert bool(hit.any()), name
    assert bool((s.weight == 0).any())


def test_reference_fuses_the_sphere_scene_to_within_a_voxel():
    S = ref.SPHERE
    origin, vs, rec, depth = ref.sphere_scene()
    r = ref.integrate_ref(S.dims, origin, vs, rec, depth, sdf_trunc=S.trunc_voxels * float(vs), depth_trunc=np.inf)
    shape = S.dims[::-1]
    m = ref.mesh_ref(r.wsum.reshape(shape).astype(np.float32), r.dsum.reshape(shape).astype(np.float32), origin, vs, 1.0)
    dist = np.abs(np.linalg.norm(m.vertices, axis=1) - S.radius) / float(vs)
    print(f"sphere scene by the reference: V = {len(m.vertices)}, F = {len(m.faces)}, largest distance {dist.max():.3f} voxel_size, mean {dist.mean():.3f}; "
          f"{int(r.ambiguous.sum())} ambiguous nodes")
    assert len(m.faces) > 3000 and float(dist.max()) < 1.0
    assert ref.topology(m.faces).manifold
