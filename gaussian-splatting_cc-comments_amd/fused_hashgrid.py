"""A multiresolution hash-grid encoding with a reproducible table gradient (include/gsr_hashgrid.h): tiny-cuda-nn's GridEncoding with
linear interpolation, in float32 -- the first half of the hash-grid + small-MLP fields of Compact-3DGS (colour), HAC (anchor context),
Grid4D and the hash-encoded (xyz, t) deformation fields, whose second half is fused_mlp.TinyMLP.

    hash_grid(x, table, levels=16, features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=2.0) -> y (N, levels * features)
    hash_grid_and_grads(x, table, dy, ...)   -> (y, dx, dtable), the raw forward and backward calls
    level_layout(D, ...)                      -> offsets, resolutions, hashed flags, total entries (host only)
    HashGrid(in_dim, levels=16, features=2, log2_hashmap_size=19, base_resolution=16, finest_resolution=None, per_level_scale=None)

    grid = HashGrid(3, levels=16, features=2, log2_hashmap_size=19, base_resolution=16, finest_resolution=4096).cuda()
    mlp = TinyMLP(grid.out_dim + 3, 3, hidden=64, hidden_layers=2, output_activation="sigmoid").cuda()
    rgb = mlp(torch.cat([grid(x01), dirs], 1))          # the Compact-3DGS colour field

x is (N, D) float32 with D in 2..4, any row stride, and is read in [0, 1]^D: every coordinate is clamped to it, and a row with a NaN or
an infinity gives zeros and takes no part in any gradient.  Mapping positions into [0, 1] (a bounding box, a scene contraction) stays
with the caller, in plain torch operations.  table is (total entries, features) float32, level-major.  The forward saves x and table
only.  The table gradient is an exact sum of 64-bit integers scaled by the largest |dy| of the call, so it has the same bits on every
run, under any permutation of the rows and for any scratch size (integer atomics: the order of integer additions cannot matter).  The
layout follows tiny-cuda-nn's so that a table trained there is meant to load here; that has not been verified against it.
HIP tensors only (no CPU path)."""
import ctypes
import math

import torch

from diff_gaussian_rasterization import _binding

MAX_LEVELS = 32          # include/gsr_hashgrid.h GSR_HASHGRID_MAX_LEVELS
MAX_LOG2_SIZE = 24       # GSR_HASHGRID_MAX_LOG2_SIZE
MAX_SCRATCH = 256 << 20  # bytes of scratch a backward takes at the most (more levels than fit run in further passes)
PATH_DIRECT, PATH_LDS = 0, 1


class HashGridDesc(ctypes.Structure):
    """gsr_hashgrid_desc"""
    _fields_ = [("N", ctypes.c_int), ("D", ctypes.c_int), ("L", ctypes.c_int), ("F", ctypes.c_int), ("base_resolution", ctypes.c_int),
                ("per_level_scale", ctypes.c_float), ("log2_hashmap_size", ctypes.c_int), ("x_stride", ctypes.c_longlong),
                ("y_stride", ctypes.c_longlong), ("dy_stride", ctypes.c_longlong), ("dx_stride", ctypes.c_longlong)]


_i, _vp, _sz, _dp = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(HashGridDesc)
_lib, _run = _binding.declare("gsr_hashgrid.h", {
    "gsr_hashgrid_layout": (_i, [_dp, _vp, _vp, _vp]),
    "gsr_hashgrid_level_scale": (ctypes.c_float, [_dp, _i]),
    "gsr_hashgrid_level_path": (_i, [_dp, _i]),
    "gsr_hashgrid_scratch_bytes": (_i, [_dp, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]),
    "gsr_hashgrid_forward": (_i, [_dp, _vp, _vp, _vp, _vp]),
    "gsr_hashgrid_backward": (_i, [_dp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}, {"gsr_hashgrid_desc": HashGridDesc})
_check_int, _check_matrix, _strided, _stride0 = _binding.check_int, _binding.check_matrix, _binding.strided, _binding.stride0


def check_config(in_dim, levels, features, log2_hashmap_size, base_resolution, per_level_scale):
    """Every refusal of a configuration, before the library is loaded -> HashGridDesc without N and strides"""
    _check_int("in_dim", in_dim, 2, 4)
    _check_int("levels", levels, 1, MAX_LEVELS)
    if isinstance(features, bool) or not isinstance(features, int):
        raise TypeError(f"features must be an int, got {features!r}")
    if features not in (1, 2, 4, 8):
        raise ValueError(f"features must be 1, 2, 4 or 8; got {features}")
    _check_int("log2_hashmap_size", log2_hashmap_size, 1, MAX_LOG2_SIZE)
    _check_int("base_resolution", base_resolution, 1, 1 << 30)
    if isinstance(per_level_scale, bool) or not isinstance(per_level_scale, (int, float)):
        raise TypeError(f"per_level_scale must be a float, got {per_level_scale!r}")
    s = ctypes.c_float(per_level_scale).value
    if not (math.isfinite(s) and s >= 1.0):
        raise ValueError(f"per_level_scale must be a finite float of at least 1; got {per_level_scale}")
    if base_resolution * s ** (levels - 1) >= 2.0 ** 30:
        raise ValueError(f"the finest resolution, base_resolution x per_level_scale^(levels - 1), must stay below 2^30; got "
                         f"{base_resolution} x {s}^{levels - 1}")
    return HashGridDesc(D=in_dim, L=levels, F=features, base_resolution=base_resolution, per_level_scale=s, log2_hashmap_size=log2_hashmap_size)


def level_layout(in_dim, levels=16, features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=2.0):
    """-> (offsets [levels + 1] in entries, resolutions [levels], hashed [levels] bools, total entries): the level table of the
    header, from the library's host code (no device is touched).  table has shape (total entries, features)."""
    d = check_config(in_dim, levels, features, log2_hashmap_size, base_resolution, per_level_scale)
    off, res, hashed = (ctypes.c_longlong * (levels + 1))(), (ctypes.c_int * levels)(), (ctypes.c_int * levels)()
    _run("gsr_hashgrid_layout", ctypes.byref(d), off, res, hashed)
    return list(off), list(res), [bool(h) for h in hashed], int(off[levels])


def level_paths(in_dim, levels=16, features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=2.0):
    """-> the table backward's path per level, PATH_LDS or PATH_DIRECT (gsr_hashgrid_level_path)"""
    d = check_config(in_dim, levels, features, log2_hashmap_size, base_resolution, per_level_scale)
    return [_lib().gsr_hashgrid_level_path(ctypes.byref(d), l) for l in range(levels)]


def _entries(d):
    """Total entries of a configuration by the header's rule in Python (the refusals must not load the library)"""
    import numpy as np
    total = 0
    with np.errstate(over="ignore"):
        for l in range(d.L):
            scale = np.float32(np.exp2(np.float64(np.float32(l) * np.float32(np.log2(np.float64(d.per_level_scale)))))) * np.float32(d.base_resolution) - np.float32(1)
            res = int(np.ceil(np.float32(scale))) + 1
            total += min((res ** d.D + 7) // 8 * 8, 1 << d.log2_hashmap_size)
    return total


def check(x, table, levels, features, log2_hashmap_size, base_resolution, per_level_scale):
    """Every refusal of the surface, before the library is loaded -> HashGridDesc without strides"""
    _check_matrix("x", x)
    _check_matrix("table", table)
    if not 2 <= x.shape[1] <= 4:
        raise ValueError(f"x must have 2, 3 or 4 columns; got {tuple(x.shape)}")
    d = check_config(int(x.shape[1]), levels, features, log2_hashmap_size, base_resolution, per_level_scale)
    if x.shape[0] >= 1 << 31:
        raise ValueError(f"x must have fewer than 2^31 rows; got {x.shape[0]}")
    if table.shape[1] != features:
        raise RuntimeError(f"table must have {features} columns (features); got {tuple(table.shape)}")
    total = _entries(d)
    if table.shape[0] != total:
        raise RuntimeError(f"table must have {total} rows, the total entries of the levels (level_layout); got {tuple(table.shape)}")
    if x.device.type != "cuda" or table.device != x.device:
        raise RuntimeError("the tensors must be HIP (cuda) tensors on one device; the hash grid has no CPU path")
    d.N = int(x.shape[0])
    return d


def _forward(d, xs, ts):
    dev = xs.device
    y = torch.empty((d.N, d.L * d.F), dtype=torch.float32, device=dev)
    if d.N == 0:
        return y
    d.x_stride, d.y_stride = _stride0(xs), _stride0(y)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        _run("gsr_hashgrid_forward", ctypes.byref(d), xs.data_ptr(), ts.data_ptr(), y.data_ptr(), stream.cuda_stream)
        for t in (xs, ts):
            t.record_stream(stream)
    return y


def _backward(d, xs, ts, dy, want_dx, want_dtable, scratch_bytes=None):
    """-> (dx or None, dtable or None).  scratch_bytes: None = the full size, capped at MAX_SCRATCH"""
    dev = xs.device
    dys = _strided(dy.detach())
    dx = torch.empty((d.N, d.D), dtype=torch.float32, device=dev) if want_dx else None
    dtable = torch.empty_like(ts) if want_dtable else None
    d.x_stride, d.dy_stride = _stride0(xs), _stride0(dys)
    d.y_stride = d.dy_stride
    d.dx_stride = d.D
    with torch.cuda.device(dev):
        nbytes = 0
        if want_dtable:
            lo, full = ctypes.c_size_t(), ctypes.c_size_t()
            _run("gsr_hashgrid_scratch_bytes", ctypes.byref(d), ctypes.byref(lo), ctypes.byref(full))
            nbytes = max(lo.value, min(full.value, MAX_SCRATCH)) if scratch_bytes is None else int(scratch_bytes)
        scratch = torch.empty((max(16, nbytes),), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        _run("gsr_hashgrid_backward", ctypes.byref(d), xs.data_ptr(), ts.data_ptr(), dys.data_ptr(), None if dx is None else dx.data_ptr(),
             None if dtable is None else dtable.data_ptr(), scratch.data_ptr(), nbytes, stream.cuda_stream)
        for t in (scratch, xs, ts, dys):
            t.record_stream(stream)
    return dx, dtable


@torch.no_grad()
def hash_grid_and_grads(x, table, dy=None, *, levels=16, features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=2.0,
                        want_dx=True, want_dtable=True, scratch_bytes=None):
    """The raw calls -> (y, dx, dtable).  dy: the gradient of y, (N, levels * features), any row stride (a column slice of a wider
    matrix is read in place), or None = the forward alone.  What is not wanted is None and is not formed.  scratch_bytes: the size of
    the backward's scratch, None = every level in one pass up to MAX_SCRATCH; the result does not depend on it."""
    d = check(x, table, levels, features, log2_hashmap_size, base_resolution, per_level_scale)
    xs, ts = _strided(x.detach()), table.detach().contiguous()
    y = _forward(d, xs, ts)
    if dy is None:
        return y, None, None
    _check_matrix("dy", dy)
    if dy.shape != y.shape or dy.device != y.device:
        raise RuntimeError(f"dy must have y's shape {tuple(y.shape)} on its device; got {tuple(dy.shape)} on {dy.device}")
    dx, dtable = _backward(d, xs, ts, dy, bool(want_dx), bool(want_dtable), scratch_bytes)
    return y, dx, dtable


class _HashGrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, table, cfg):
        d = check(x, table, *cfg)
        xs, ts = _strided(x.detach()), table.detach().contiguous()
        ctx.cfg = cfg
        ctx.save_for_backward(xs, ts)   # x and the table: nothing of size N x levels is kept
        return _forward(d, xs, ts)

    @staticmethod
    def backward(ctx, dy):
        xs, ts = ctx.saved_tensors
        d = check(xs, ts, *ctx.cfg)
        if d.N == 0:
            return (torch.zeros_like(xs) if ctx.needs_input_grad[0] else None), (torch.zeros_like(ts) if ctx.needs_input_grad[1] else None), None
        dx, dtable = _backward(d, xs, ts, dy, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dx, dtable, None


def hash_grid(x, table, levels=16, features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=2.0):
    """y (N, levels * features) = the encoding of the module docstring of every row of x; differentiable w.r.t. table, and w.r.t. x
    where x requires a gradient (each is formed only where it is required)."""
    cfg = (levels, features, log2_hashmap_size, base_resolution, per_level_scale)
    check(x, table, *cfg)
    return _HashGrid.apply(x, table, cfg)


class HashGrid(torch.nn.Module):
    """The encoding as a module with one parameter, table (total entries, features), initialised U(-1e-4, 1e-4) as tiny-cuda-nn does;
    [module.table] is one FusedAdam group.  The growth factor is given by per_level_scale, or by finest_resolution as
    exp(log(finest_resolution / base_resolution) / (levels - 1)); with neither it is 2.  out_dim = levels * features.

        grid = HashGrid(3, levels=16, features=2, log2_hashmap_size=19, base_resolution=16, finest_resolution=4096).cuda()
        mlp = TinyMLP(grid.out_dim + 3, 3, hidden=64, hidden_layers=2, output_activation="sigmoid").cuda()
        rgb = mlp(torch.cat([grid(x01), dirs], 1))      # the Compact-3DGS colour field; x01 = positions mapped into [0, 1]^3 by the caller
    """

    def __init__(self, in_dim, levels=16, features=2, log2_hashmap_size=19, base_resolution=16, finest_resolution=None, per_level_scale=None):
        super().__init__()
        if finest_resolution is not None and per_level_scale is not None:
            raise ValueError("give finest_resolution or per_level_scale, not both")
        _check_int("levels", levels, 1, MAX_LEVELS)
        _check_int("base_resolution", base_resolution, 1, 1 << 30)
        if finest_resolution is not None:
            _check_int("finest_resolution", finest_resolution, base_resolution, 1 << 30)
            per_level_scale = math.exp(math.log(finest_resolution / base_resolution) / (levels - 1)) if levels > 1 else 1.0
        elif per_level_scale is None:
            per_level_scale = 2.0
        d = check_config(in_dim, levels, features, log2_hashmap_size, base_resolution, per_level_scale)
        self.in_dim, self.levels, self.features, self.log2_hashmap_size = in_dim, levels, features, log2_hashmap_size
        self.base_resolution, self.per_level_scale = base_resolution, d.per_level_scale
        self.out_dim = levels * features
        self.table = torch.nn.Parameter(torch.empty((_entries(d), features), dtype=torch.float32).uniform_(-1e-4, 1e-4))

    def forward(self, x):
        return hash_grid(x, self.table, self.levels, self.features, self.log2_hashmap_size, self.base_resolution, self.per_level_scale)

    def extra_repr(self):
        return (f"in_dim={self.in_dim}, levels={self.levels}, features={self.features}, log2_hashmap_size={self.log2_hashmap_size}, "
                f"base_resolution={self.base_resolution}, per_level_scale={self.per_level_scale:.6g}, entries={self.table.shape[0]}")
