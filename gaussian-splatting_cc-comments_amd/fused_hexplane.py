"""A HexPlane / K-Planes plane-grid encoding with a reproducible table gradient (include/gsr_hexplane.h): a point (x, y, z[, t]) is
projected onto every pair of axes, each projection interpolates bilinearly in a small 2-D feature plane (F.grid_sample with
align_corners=True and border padding), and the per-plane features are multiplied together, at several resolutions -- the first half
of the deformation fields of 4DGaussians, the K-Planes fields and tri-plane context models, whose second half is fused_mlp.TinyMLP.

    cfg = HexPlaneConfig(in_dim=4, channels=32, res=resolutions((64, 64, 64, 25), (1, 2)), concat=True)
    hex_plane(x, table, cfg)                       -> y (N, L * C), or (N, C) with concat=False (the sum over the levels)
    hex_plane_and_grads(x, table, dy, cfg, ...)    -> (y, dx, dtable), the raw forward and backward calls
    plane_layout(cfg), level_paths(cfg)            -> where each plane lies in table, and its path in the table backward (host only)
    pack_planes(grids), unpack_planes(table, cfg)  <-> the list (levels) of lists (planes) of (1, C, res_b, res_a) tensors of K-Planes code
    plane_regularizer(table, cfg, tv_space=..)     -> total variation, time smoothness and |1 - v| of the planes, differentiable in table
    HexPlane(in_dim=4, channels=32, base=(64, 64, 64, 25), multires=(1, 2), concat=True, aabb=None)

    field = HexPlane(4, channels=32, aabb=scene_box).cuda()
    mlp = TinyMLP(field.out_dim, 10, hidden=64, hidden_layers=2).cuda()
    offsets = mlp(field(torch.cat([xyz, t], 1)))            # the 4DGaussians deformation field

x is (N, D) float32 with D in {3, 4}, any row stride, and is read in [-1, 1]^D: a coordinate beyond it reads the border node, and a row
with a NaN or an infinity gives zeros and takes no part in any gradient.  The planes are the axis pairs (a, b), a < b, in
itertools.combinations order; table is one flat float32 tensor, level-major, then the planes, each [res_b][res_a][C] (channels last).
The forward saves x and table only.  The table gradient is an exact sum of 64-bit integers, scaled from the largest |dy| of the call and
the largest |v| of every plane, so it has the same bits on every run, under any permutation of the rows and for any scratch size.
HIP tensors only (no CPU path)."""
import ctypes
import itertools

import torch

from diff_gaussian_rasterization import _binding

MAX_LEVELS = 8           # include/gsr_hexplane.h GSR_HEXPLANE_MAX_LEVELS
MAX_RES = 4096           # GSR_HEXPLANE_MAX_RES
LDS_BYTES = 128 * 1024   # GSR_HEXPLANE_LDS_BYTES
REG_SCRATCH = 65536      # GSR_HEXPLANE_REG_SCRATCH_BYTES
MAX_SCRATCH = 256 << 20  # bytes of scratch a backward takes at the most (more planes than fit run in further passes)
PATH_DIRECT, PATH_LDS = 0, 1


class HexPlaneDesc(ctypes.Structure):
    """gsr_hexplane_desc"""
    _fields_ = [("N", ctypes.c_int), ("D", ctypes.c_int), ("L", ctypes.c_int), ("C", ctypes.c_int), ("concat", ctypes.c_int),
                ("res", (ctypes.c_int * 4) * MAX_LEVELS), ("x_stride", ctypes.c_longlong), ("y_stride", ctypes.c_longlong),
                ("dy_stride", ctypes.c_longlong), ("dx_stride", ctypes.c_longlong)]


_i, _f, _vp, _sz, _dp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(HexPlaneDesc)
_lib, _run = _binding.declare("gsr_hexplane.h", {
    "gsr_hexplane_layout": (_i, [_dp, _vp]),
    "gsr_hexplane_level_path": (_i, [_dp, _i, _i]),
    "gsr_hexplane_scratch_bytes": (_i, [_dp, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]),
    "gsr_hexplane_forward": (_i, [_dp, _vp, _vp, _vp, _vp]),
    "gsr_hexplane_backward": (_i, [_dp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gsr_hexplane_regularizer": (_i, [_dp, _vp, _f, _f, _f, _f, _f, _vp, _vp, _vp, _sz, _vp]),
}, {"gsr_hexplane_desc": HexPlaneDesc})
_check_int, _check_matrix, _check_number, _strided, _stride0 = (_binding.check_int, _binding.check_matrix, _binding.check_number,
                                                                 _binding.strided, _binding.stride0)


def resolutions(base=(64, 64, 64, 25), multires=(1, 2)):
    """-> one resolution per level and axis, ((r_0, .., r_{D-1}), ..): the spatial axes 0..2 scaled by each factor, the time axis kept"""
    for m in multires:
        _check_int("a factor of multires", m, 1)
    for r in base:
        _check_int("a resolution of base", r, 2)
    return tuple(tuple(r * m if a < 3 else r for a, r in enumerate(base)) for m in multires)


class HexPlaneConfig:
    """What a table means: in_dim (D) input columns, channels (C), res[l][a] and whether the levels are concatenated or summed.
    Every refusal of a configuration happens here, before the library is loaded."""

    def __init__(self, in_dim=4, channels=32, res=None, concat=True):
        _check_int("in_dim", in_dim, 3, 4)
        _check_int("channels", channels, 4, 64)
        if channels % 4:
            raise ValueError(f"channels must be a multiple of 4 in 4..64; got {channels}")
        res = resolutions(tuple((64, 64, 64, 25)[:in_dim])) if res is None else res
        if not isinstance(res, (tuple, list)) or not all(isinstance(r, (tuple, list)) for r in res):
            raise TypeError(f"res must be a sequence (levels) of sequences (axes) of ints, got {res!r}")
        _check_int("the number of levels (len(res))", len(res), 1, MAX_LEVELS)
        for level in res:
            if len(level) != in_dim:
                raise ValueError(f"every level of res must give {in_dim} resolutions (in_dim); got {tuple(level)}")
            for r in level:
                _check_int("a resolution", r, 2, MAX_RES)
        self.in_dim, self.channels, self.concat = in_dim, channels, bool(concat)
        self.res = tuple(tuple(level) for level in res)
        self.levels = len(self.res)
        self.planes = tuple(itertools.combinations(range(in_dim), 2))
        self.out_dim = self.levels * channels if self.concat else channels

    def key(self):
        return (self.in_dim, self.channels, self.res, self.concat)

    def __eq__(self, other):
        return isinstance(other, HexPlaneConfig) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return f"HexPlaneConfig(in_dim={self.in_dim}, channels={self.channels}, res={self.res}, concat={self.concat})"

    def shapes(self):
        """-> [(level, plane, (a, b), res_b, res_a)] in the table's order"""
        return [(l, k, ab, self.res[l][ab[1]], self.res[l][ab[0]]) for l in range(self.levels) for k, ab in enumerate(self.planes)]

    def total(self):
        """The floats of a table, by the header's rule in Python (the refusals must not load the library)"""
        return sum(rb * ra * self.channels for _, _, _, rb, ra in self.shapes())

    def desc(self, N=0):
        d = HexPlaneDesc(N=N, D=self.in_dim, L=self.levels, C=self.channels, concat=int(self.concat))
        for l, level in enumerate(self.res):
            for a, r in enumerate(level):
                d.res[l][a] = r
        return d


def _config(cfg):
    if not isinstance(cfg, HexPlaneConfig):
        raise TypeError(f"cfg must be a HexPlaneConfig, got {type(cfg).__name__}")
    return cfg


def plane_layout(cfg):
    """-> (offsets [levels * planes + 1] in floats, shapes [(res_b, res_a)] per plane in the table's order, total floats): from the
    library's host code (no device is touched).  Plane k of level l is table[off : off + res_b * res_a * C].view(res_b, res_a, C)."""
    cfg = _config(cfg)
    n = cfg.levels * len(cfg.planes)
    off = (ctypes.c_longlong * (n + 1))()
    _run("gsr_hexplane_layout", ctypes.byref(cfg.desc()), off)
    return list(off), [(rb, ra) for _, _, _, rb, ra in cfg.shapes()], int(off[n])


def level_paths(cfg):
    """-> [level][plane] the table backward's path, PATH_LDS or PATH_DIRECT (gsr_hexplane_level_path)"""
    d = _config(cfg).desc()
    return [[_lib().gsr_hexplane_level_path(ctypes.byref(d), l, k) for k in range(len(cfg.planes))] for l in range(cfg.levels)]


def pack_planes(grids):
    """grids[l][k]: (1, C, res_b, res_a) tensors, the planes of level l in itertools.combinations order -> the flat table"""
    return torch.cat([g[0].permute(1, 2, 0).reshape(-1) for level in grids for g in level])


def unpack_planes(table, cfg):
    """The flat table -> grids[l][k] of shape (1, C, res_b, res_a) (views of table where it is contiguous)"""
    cfg = _config(cfg)
    if table.dim() != 1 or table.shape[0] != cfg.total():
        raise RuntimeError(f"table must be one flat tensor of {cfg.total()} elements (plane_layout); got {tuple(table.shape)}")
    grids, off = [[] for _ in range(cfg.levels)], 0
    for l, _, _, rb, ra in cfg.shapes():
        n = rb * ra * cfg.channels
        grids[l].append(table[off:off + n].view(rb, ra, cfg.channels).permute(2, 0, 1)[None])
        off += n
    return grids


def _check_table(table, cfg):
    if not torch.is_tensor(table):
        raise TypeError("table must be a tensor")
    if table.dim() != 1 or table.shape[0] != cfg.total():
        raise RuntimeError(f"table must be one flat tensor of {cfg.total()} elements (plane_layout); got {tuple(table.shape)}")
    if table.dtype != torch.float32:
        raise RuntimeError(f"table must be float32; got {table.dtype}")


def check(x, table, cfg):
    """Every refusal of the surface, before the library is loaded -> HexPlaneDesc without strides"""
    cfg = _config(cfg)
    _check_matrix("x", x)
    if x.shape[1] != cfg.in_dim:
        raise ValueError(f"x must have {cfg.in_dim} columns (in_dim); got {tuple(x.shape)}")
    if x.shape[0] >= 1 << 31:
        raise ValueError(f"x must have fewer than 2^31 rows; got {x.shape[0]}")
    _check_table(table, cfg)
    if x.device.type != "cuda" or table.device != x.device:
        raise RuntimeError("the tensors must be HIP (cuda) tensors on one device; the plane grid has no CPU path")
    return cfg.desc(int(x.shape[0]))


def _forward(d, cfg, xs, ts):
    dev = xs.device
    y = torch.empty((d.N, cfg.out_dim), dtype=torch.float32, device=dev)
    if d.N == 0:
        return y
    d.x_stride, d.y_stride = _stride0(xs), _stride0(y)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        _run("gsr_hexplane_forward", ctypes.byref(d), xs.data_ptr(), ts.data_ptr(), y.data_ptr(), stream.cuda_stream)
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
            _run("gsr_hexplane_scratch_bytes", ctypes.byref(d), ctypes.byref(lo), ctypes.byref(full))
            nbytes = max(lo.value, min(full.value, MAX_SCRATCH)) if scratch_bytes is None else int(scratch_bytes)
        scratch = torch.empty((max(16, nbytes),), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        _run("gsr_hexplane_backward", ctypes.byref(d), xs.data_ptr(), ts.data_ptr(), dys.data_ptr(), None if dx is None else dx.data_ptr(),
             None if dtable is None else dtable.data_ptr(), scratch.data_ptr(), nbytes, stream.cuda_stream)
        for t in (scratch, xs, ts, dys):
            t.record_stream(stream)
    return dx, dtable


@torch.no_grad()
def hex_plane_and_grads(x, table, dy, cfg, want_dx=True, want_dtable=True, scratch_bytes=None):
    """The raw calls -> (y, dx, dtable).  dy: the gradient of y, y's shape, any row stride (a column slice of a wider matrix is read
    in place), or None = the forward alone.  What is not wanted is None and is not formed.  scratch_bytes: the size of the backward's
    scratch, None = every plane in one pass up to MAX_SCRATCH; the result does not depend on it."""
    d = check(x, table, cfg)
    xs, ts = _strided(x.detach()), table.detach().contiguous()
    y = _forward(d, cfg, xs, ts)
    if dy is None:
        return y, None, None
    _check_matrix("dy", dy)
    if dy.shape != y.shape or dy.device != y.device:
        raise RuntimeError(f"dy must have y's shape {tuple(y.shape)} on its device; got {tuple(dy.shape)} on {dy.device}")
    if d.N == 0:
        return y, (torch.zeros_like(xs) if want_dx else None), (torch.zeros_like(ts) if want_dtable else None)
    dx, dtable = _backward(d, xs, ts, dy, bool(want_dx), bool(want_dtable), scratch_bytes)
    return y, dx, dtable


class _HexPlane(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, table, cfg):
        d = check(x, table, cfg)
        xs, ts = _strided(x.detach()), table.detach().contiguous()
        ctx.cfg = cfg
        ctx.save_for_backward(xs, ts)   # x and the table: nothing of size N x levels x planes is kept
        return _forward(d, cfg, xs, ts)

    @staticmethod
    def backward(ctx, dy):
        xs, ts = ctx.saved_tensors
        d = check(xs, ts, ctx.cfg)
        if d.N == 0:
            return (torch.zeros_like(xs) if ctx.needs_input_grad[0] else None), (torch.zeros_like(ts) if ctx.needs_input_grad[1] else None), None
        dx, dtable = _backward(d, xs, ts, dy, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dx, dtable, None


def hex_plane(x, table, cfg):
    """y = the encoding of the module docstring of every row of x; differentiable w.r.t. table, and w.r.t. x where x requires a
    gradient (each is formed only where it is required)."""
    check(x, table, cfg)
    return _HexPlane.apply(x, table, cfg)


# ---- the regulariser ---------------------------------------------------------------------------------------------------------------
def _regularizer(table, cfg, weights, want_dtable):
    """-> (value, a 0-d tensor; dtable or None)"""
    d = cfg.desc()
    dev = table.device
    ts = table.detach().contiguous()
    value = torch.empty((), dtype=torch.float32, device=dev)
    dtable = torch.empty_like(ts) if want_dtable else None
    with torch.cuda.device(dev):
        scratch = torch.empty((REG_SCRATCH,), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        _run("gsr_hexplane_regularizer", ctypes.byref(d), ts.data_ptr(), *weights, value.data_ptr(), None if dtable is None else dtable.data_ptr(),
             scratch.data_ptr(), REG_SCRATCH, stream.cuda_stream)
        for t in (scratch, ts):
            t.record_stream(stream)
    return value, dtable


class _Regularizer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, cfg, weights):
        value, dtable = _regularizer(table, cfg, weights, ctx.needs_input_grad[0])
        ctx.save_for_backward(dtable)
        return value

    @staticmethod
    def backward(ctx, dvalue):
        (dtable,) = ctx.saved_tensors
        return dtable * dvalue, None, None


def plane_regularizer(table, cfg, tv_space=0.0, tv_time=0.0, smooth_space=0.0, smooth_time=0.0, l1_time=0.0):
    """tv_space * sum tv + smooth_space * sum smooth over the planes without the time axis, plus tv_time * sum tv + smooth_time * sum
    smooth + l1_time * sum mean|1 - v| over the time planes, each sum over the levels (include/gsr_hexplane.h: K-Planes' plane TV,
    its time smoothness -- the second difference along a plane's slow axis -- and its L1 pull of the time planes to 1) -> a 0-d
    tensor, differentiable in table.  One pass and a fixed-order fold: the same bits on every run."""
    cfg = _config(cfg)
    _check_table(table, cfg)
    weights = tuple(_check_number(n, v) for n, v in (("tv_space", tv_space), ("tv_time", tv_time), ("smooth_space", smooth_space),
                                                     ("smooth_time", smooth_time), ("l1_time", l1_time)))
    if table.device.type != "cuda":
        raise RuntimeError("the tensors must be HIP (cuda) tensors on one device; the plane grid has no CPU path")
    return _Regularizer.apply(table, cfg, weights)


# ---- the module --------------------------------------------------------------------------------------------------------------------
class HexPlane(torch.nn.Module):
    """The encoding as a module with one parameter, table (flat; [module.table] is one FusedAdam group), initialised to 1 on the time
    planes and U(0.1, 0.5) elsewhere, as K-Planes and 4DGaussians do.  aabb: None, or ((min_0, ..), (max_0, ..)) over the first
    len(min) columns of x, which are mapped from the box to [-1, 1] in plain torch before the encoding (the other columns -- the time
    of a 3-D box -- are taken as they are).  out_dim = levels * channels, or channels with concat=False.

        field = HexPlane(4, channels=32, base=(64, 64, 64, 25), multires=(1, 2), aabb=((-1.3, -1.3, -1.3), (1.3, 1.3, 1.3))).cuda()
        feats = field(torch.cat([xyz, t * 2 - 1], 1))
        loss = loss + field.regularizer(tv_space=2e-4, tv_time=2e-4, smooth_time=1e-3, l1_time=1e-4)
    """

    def __init__(self, in_dim=4, channels=32, base=(64, 64, 64, 25), multires=(1, 2), concat=True, aabb=None):
        super().__init__()
        _check_int("in_dim", in_dim, 3, 4)
        if len(base) < in_dim:
            raise ValueError(f"base must give {in_dim} resolutions (in_dim); got {tuple(base)}")
        self.cfg = HexPlaneConfig(in_dim, channels, resolutions(tuple(base[:in_dim]), multires), concat)
        self.in_dim, self.channels, self.out_dim = in_dim, channels, self.cfg.out_dim
        grids = [[] for _ in range(self.cfg.levels)]
        for l, _, (a, b), rb, ra in self.cfg.shapes():
            g = torch.empty((1, channels, rb, ra), dtype=torch.float32)
            grids[l].append(g.fill_(1.0) if b == 3 else g.uniform_(0.1, 0.5))
        self.table = torch.nn.Parameter(pack_planes(grids))
        if aabb is not None:
            lo, hi = (torch.as_tensor(v, dtype=torch.float32).reshape(-1) for v in aabb)
            if lo.shape != hi.shape or not 1 <= lo.shape[0] <= in_dim or not bool((hi > lo).all()):
                raise ValueError(f"aabb must be (min, max) over at most {in_dim} columns with max > min; got {aabb!r}")
            self.register_buffer("aabb_min", lo)
            self.register_buffer("aabb_scale", 2.0 / (hi - lo))
        else:
            self.aabb_min = self.aabb_scale = None

    def forward(self, x):
        if self.aabb_min is not None:
            n = self.aabb_min.shape[0]
            head = (x[:, :n] - self.aabb_min) * self.aabb_scale - 1.0
            x = head if n == x.shape[1] else torch.cat([head, x[:, n:]], 1)
        return hex_plane(x, self.table, self.cfg)

    def regularizer(self, tv_space=0.0, tv_time=0.0, smooth_space=0.0, smooth_time=0.0, l1_time=0.0):
        return plane_regularizer(self.table, self.cfg, tv_space, tv_time, smooth_space, smooth_time, l1_time)

    def extra_repr(self):
        return f"in_dim={self.in_dim}, channels={self.channels}, res={self.cfg.res}, concat={self.cfg.concat}, floats={self.table.shape[0]}"
