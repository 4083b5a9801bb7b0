"""TSDF fusion of rendered depth maps and mesh extraction as fused HIP kernels (include/gsr_tsdf.h): the step the geometry-regularised
methods (2DGS, PGSR, RaDe-GS, Gaussian surfels) end with, which they take from Open3D's TSDF volumes and marching cubes:

    vol = TSDFVolume(origin, voxel_size, dims=(NX, NY, NZ))      a dense volume of sums: weight, weight * tsdf, weight * rgb
    vol.integrate(depth, cameras, color=None, weight=None)       one launch for the whole batch of views: a thread per node walks the cameras
    vol.tsdf(), vol.weight()                                     (NZ, NY, NX) views of the field
    vol.extract_mesh(min_weight=1.0)                             marching tetrahedra -> (vertices (V,3), faces (F,3) int32, colors (V,3) or None)
    vol.reset()
    TSDFVolume.from_planes(origin, voxel_size, wsum, dsum)       a volume around planes of the caller's making, such as an SDF of its own

    vol = TSDFVolume(origin=(-2, -2, -2), voxel_size=4 / 255, dims=(256, 256, 256), device="cuda")
    for cam in train_cameras:
        out = render(cam, pc, pipe, bg, depth_alpha="depth", median_depth=True)
        alpha = out["alpha"]
        vol.integrate(out["median_depth"], [cam], color=out["render"], weight=(alpha > 0.5).float())
    vertices, faces, colors = vol.extract_mesh()
    gsr_ply.write_mesh_ply("mesh.ply", vertices, faces, colors)

Rendering all views first and integrating them in one call reads and writes the volume once instead of once per view; the result has
the same bits either way (the sums run in ascending camera order).  The mesh is bit-identical from run to run: no atomics anywhere.
What stays with the caller: choosing the bounds and the resolution of the volume; keeping the largest connected components of the
mesh, or decimating it (marching tetrahedra gives about twice the triangles of marching cubes, and no holes); fisheye cameras
(fused_filter3d.pack_cameras raises NotImplementedError for them).  HIP tensors only (no CPU fallback).
"""
import ctypes
import functools
import math

import torch

from diff_gaussian_rasterization import _binding
from fused_filter3d import CAMERA_FLOATS, _camera_scalars, pack_cameras

THREADS = 256            # include/gsr_tsdf.h GSR_TSDF_THREADS
PLAN_MAGIC = 0x74736466  # GSR_TSDF_PLAN_MAGIC


class Grid(ctypes.Structure):       # include/gsr_tsdf.h gsr_tsdf_grid
    _fields_ = [("nx", ctypes.c_int), ("ny", ctypes.c_int), ("nz", ctypes.c_int), ("origin", ctypes.c_float * 3), ("voxel_size", ctypes.c_float)]


class MeshPlan(ctypes.Structure):   # gsr_tsdf_mesh_plan_t
    _fields_ = [("V", ctypes.c_longlong), ("F", ctypes.c_longlong), ("grid", Grid), ("wsum", ctypes.c_void_p), ("dsum", ctypes.c_void_p),
                ("scratch", ctypes.c_void_p), ("min_weight", ctypes.c_float), ("magic", ctypes.c_int)]


_i, _f, _ll, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_longlong, ctypes.c_void_p
_lib, _run = _binding.declare("gsr_tsdf.h", {
    "gsr_tsdf_integrate": (_i, [ctypes.POINTER(Grid), _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _f, _f, _vp]),
    "gsr_tsdf_mesh_scratch_bytes": (ctypes.c_size_t, [_ll]),
    "gsr_tsdf_mesh_plan": (_i, [ctypes.POINTER(Grid), _vp, _vp, _f, _vp, ctypes.POINTER(MeshPlan), _vp]),
    "gsr_tsdf_mesh_emit": (_i, [ctypes.POINTER(MeshPlan), _ll, _ll, _vp, _vp, _vp, _vp, _vp]),
}, {"gsr_tsdf_grid": Grid, "gsr_tsdf_mesh_plan_t": MeshPlan})
_ptr = _binding.ptr
_check_device = functools.partial(_binding.check_device, "TSDF kernels")


def _positive(name, v):
    x = _binding.check_number(name, v, "a number", repr)
    if not (math.isfinite(x) and x > 0.0):
        raise ValueError(f"{name} must be finite and positive; got {v}")
    return x


class TSDFVolume:
    """A dense truncated signed distance field on NX x NY x NZ sample points at origin + (i, j, k) voxel_size, held as sums on the device:
    wsum, dsum = sum w tsdf and, with color=True, csum = sum w rgb, each (NZ, NY, NX) float32 (csum (3, NZ, NY, NX)); the attributes of
    those names are the planes themselves.  sdf_trunc: the truncation distance, 4 voxel_size where None.  depth_trunc: depths beyond it
    are ignored."""

    def __init__(self, origin, voxel_size, dims, sdf_trunc=None, depth_trunc=math.inf, color=True, device="cuda"):
        self._setup(origin, voxel_size, dims, sdf_trunc, depth_trunc)
        if not isinstance(color, bool):
            raise TypeError(f"color must be True or False, got {color!r}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("the volume lives on a HIP (cuda) device; the TSDF kernels have no CPU path")
        shape = self.dims[::-1]
        self.wsum = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.dsum = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.csum = torch.zeros((3,) + shape, dtype=torch.float32, device=dev) if color else None

    def _setup(self, origin, voxel_size, dims, sdf_trunc, depth_trunc):
        origin = tuple(float(v) for v in origin)
        if len(origin) != 3 or not all(math.isfinite(v) for v in origin):
            raise ValueError(f"origin must be three finite numbers; got {origin}")
        dims = tuple(dims)
        if len(dims) != 3 or not all(isinstance(n, int) and not isinstance(n, bool) and n >= 1 for n in dims):
            raise ValueError(f"dims must be three integers (NX, NY, NZ), each at least 1; got {dims}")
        if dims[0] * dims[1] * dims[2] > 2 ** 31 - 1:
            raise ValueError(f"dims {dims}: the volume must have fewer than 2^31 nodes")
        self.origin, self.dims = origin, dims
        self.voxel_size = _positive("voxel_size", voxel_size)
        self.sdf_trunc = 4.0 * self.voxel_size if sdf_trunc is None else _positive("sdf_trunc", sdf_trunc)
        if isinstance(depth_trunc, bool) or not isinstance(depth_trunc, (int, float)) or not depth_trunc > 0.0:
            raise ValueError(f"depth_trunc must be positive (inf: no limit); got {depth_trunc!r}")
        self.depth_trunc = float(depth_trunc)

    @classmethod
    def from_planes(cls, origin, voxel_size, wsum, dsum, csum=None, sdf_trunc=None, depth_trunc=math.inf):
        """A volume around the caller's planes, adopted and not copied: wsum and dsum (NZ, NY, NX) float32 and contiguous on the device,
        csum (3, NZ, NY, NX) or None.  A signed distance field of one's own goes in as dsum = value, wsum = 1 where it is known."""
        for n, t in (("wsum", wsum), ("dsum", dsum)) + ((("csum", csum),) if csum is not None else ()):
            if not torch.is_tensor(t):
                raise TypeError(f"{n} must be a tensor")
            if t.dtype != torch.float32:
                raise RuntimeError(f"{n} must be float32; got {t.dtype}")
            if not t.is_contiguous():
                raise RuntimeError(f"{n} is adopted and changed in place and must be contiguous")
        if wsum.dim() != 3 or dsum.shape != wsum.shape or (csum is not None and tuple(csum.shape) != (3,) + tuple(wsum.shape)):
            raise RuntimeError(f"wsum and dsum must be (NZ, NY, NX) and csum (3, NZ, NY, NX); got {tuple(wsum.shape)}, {tuple(dsum.shape)}"
                               + ("" if csum is None else f", {tuple(csum.shape)}"))
        self = cls.__new__(cls)
        self._setup(origin, voxel_size, tuple(int(n) for n in wsum.shape[::-1]), sdf_trunc, depth_trunc)
        _check_device(*(t for t in (wsum, dsum, csum) if t is not None))
        self.wsum, self.dsum, self.csum = wsum, dsum, csum
        return self

    def _grid(self):
        return Grid(self.dims[0], self.dims[1], self.dims[2], (ctypes.c_float * 3)(*self.origin), self.voxel_size)

    @torch.no_grad()
    def integrate(self, depth, cameras, color=None, weight=None):
        """Fuses C depth maps.  depth: (C,H,W) or (C,1,H,W), or (H,W) / (1,H,W) with one camera: the distance along the camera's z axis, as
        `depth` and `median_depth` of the renderer; pixels that are 0, negative, not finite or beyond depth_trunc are ignored.  cameras: a
        list of C cameras or the packed (C, 20) tensor of fused_filter3d.pack_cameras (read back here to compare the image sizes; a list
        costs no read-back).  color: (C,3,H,W) or (3,H,W), needs a volume with color=True.  weight: as depth; pixels with weight <= 0 are
        ignored -- the place for an alpha mask.  float32 on the volume's device, any strides.  -> self"""
        if not torch.is_tensor(depth):
            raise TypeError("depth must be a tensor")
        if torch.is_tensor(cameras):
            if cameras.dim() != 2 or cameras.shape[0] < 1 or cameras.shape[1] != CAMERA_FLOATS or cameras.dtype != torch.float32:
                raise RuntimeError(f"cameras must be a float32 (C, {CAMERA_FLOATS}) tensor with C >= 1 (pack_cameras); got {cameras.dtype} "
                                   f"{tuple(cameras.shape)}")
            C = int(cameras.shape[0])
        else:
            _camera_scalars(cameras)
            C = len(cameras)
        if depth.dim() == 4 and depth.shape[1] == 1:
            depth = depth[:, 0]
        elif depth.dim() == 2:
            depth = depth[None]
        if depth.dim() != 3 or depth.shape[0] != C or depth.shape[1] < 1 or depth.shape[2] < 1:
            raise RuntimeError(f"depth must be (C,H,W) or (C,1,H,W) for the {C} cameras, or (H,W) with one; got {tuple(depth.shape)}")
        H, W = int(depth.shape[1]), int(depth.shape[2])
        named = [("depth", depth)]
        if weight is not None:
            if not torch.is_tensor(weight):
                raise TypeError("weight must be a tensor")
            weight = weight.reshape(depth.shape) if weight.numel() == depth.numel() else weight
            if weight.shape != depth.shape:
                raise RuntimeError(f"weight must have the shape of depth {tuple(depth.shape)}; got {tuple(weight.shape)}")
            named.append(("weight", weight))
        if color is not None:
            if not torch.is_tensor(color):
                raise TypeError("color must be a tensor")
            if self.csum is None:
                raise RuntimeError("color needs a volume made with color=True")
            if color.dim() == 3 and C == 1:
                color = color[None]
            if tuple(color.shape) != (C, 3, H, W):
                raise RuntimeError(f"color must be (C,3,H,W) = {(C, 3, H, W)}; got {tuple(color.shape)}")
            named.append(("color", color))
        for n, t in named:
            if t.dtype != torch.float32:
                raise RuntimeError(f"{n} must be float32; got {t.dtype}")
        dev = _check_device(self.wsum, *(t for _, t in named), *((cameras,) if torch.is_tensor(cameras) else ()))
        host = cameras.detach().cpu().contiguous() if torch.is_tensor(cameras) else pack_cameras(cameras, "cpu")
        for c in range(C):
            if float(host[c, 16]) != W or float(host[c, 17]) != H:
                raise RuntimeError(f"camera {c} is {float(host[c, 16]):g} x {float(host[c, 17]):g}, the depth maps are {W} x {H}")
        with torch.cuda.device(dev):
            cams = cameras.detach().contiguous() if torch.is_tensor(cameras) else host.to(dev)
            d = depth.detach().contiguous()
            w = None if weight is None else weight.detach().contiguous()
            rgb = None if color is None else color.detach().contiguous()
            stream = torch.cuda.current_stream(dev)
            _run("gsr_tsdf_integrate", ctypes.byref(self._grid()), self.wsum.data_ptr(), self.dsum.data_ptr(), _ptr(self.csum), C, cams.data_ptr(),
                 host.data_ptr(), H, W, d.data_ptr(), _ptr(rgb), _ptr(w), self.sdf_trunc, self.depth_trunc, stream.cuda_stream)
            for t in (cams, d, w, rgb):
                if t is not None:
                    t.record_stream(stream)
        return self

    def weight(self):
        """-> wsum (NZ, NY, NX): the plane itself"""
        return self.wsum

    def tsdf(self):
        """-> dsum / wsum (NZ, NY, NX), NaN where the weight is 0"""
        return torch.where(self.wsum > 0, self.dsum / self.wsum, torch.full_like(self.dsum, float("nan")))

    def reset(self):
        for t in (self.wsum, self.dsum, self.csum):
            if t is not None:
                t.zero_()
        return self

    @torch.no_grad()
    def extract_mesh(self, min_weight=1.0):
        """Marching tetrahedra over the nodes with wsum >= min_weight -> (vertices (V,3) float32, faces (F,3) int32, colors (V,3) float32 or
        None without colour planes).  Every cell is cut into the six tetrahedra around its main diagonal; a vertex lies on every grid edge
        (axis, face diagonal or cell diagonal) whose ends are valid and on different sides of 0, at t = v0 / (v0 - v1); faces are
        counter-clockwise seen from free space.  Vertices ascend in (node, edge kind), faces in (cell, tetrahedron, triangle): the mesh is
        the same from run to run, bit for bit.  An empty mesh is (0,3) tensors.  One read-back of the two counts."""
        min_weight = _positive("min_weight", min_weight)
        if min(self.dims) < 2:
            raise ValueError(f"extraction needs at least 2 nodes along every axis; the volume is {self.dims}")
        dev = _check_device(self.wsum)
        lib = _lib()
        nodes = self.dims[0] * self.dims[1] * self.dims[2]
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            scratch = torch.empty(lib.gsr_tsdf_mesh_scratch_bytes(nodes), dtype=torch.uint8, device=dev)
            plan = MeshPlan()
            _run("gsr_tsdf_mesh_plan", ctypes.byref(self._grid()), self.wsum.data_ptr(), self.dsum.data_ptr(), min_weight, scratch.data_ptr(),
                 ctypes.byref(plan), stream.cuda_stream)
            V, F = int(plan.V), int(plan.F)
            if V > 2 ** 31 - 1 or F > 2 ** 31 - 1:
                raise RuntimeError(f"the mesh has {V} vertices and {F} faces: beyond 2^31 - 1; extract the volume in parts")
            vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
            faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
            colors = None if self.csum is None else torch.empty((V, 3), dtype=torch.float32, device=dev)
            _run("gsr_tsdf_mesh_emit", ctypes.byref(plan), V, F, _ptr(self.csum), vertices.data_ptr(), _ptr(colors), faces.data_ptr(), stream.cuda_stream)
            scratch.record_stream(stream)
        return vertices, faces, colors
