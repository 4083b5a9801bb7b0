"""The neighbour graph of the Gaussians as fused HIP kernels (include/gsr_knn.h): an exact K-nearest-neighbour search that returns
indices, for any K up to 32 and an optional second point set, and a neighbour gather whose backward is bitwise reproducible -- what
SuGaR (16 neighbours, rebuilt during training), Dynamic 3D Gaussians (20 neighbours for the rigidity, rotation and isometry losses),
the isometry / physics regularisers and statistical outlier pruning need, and what simple_knn.distCUDA2 does not return:

    knn(points, K, queries=None)         -> (dist2 (Q,K) float32 ascending, idx (Q,K) int32 into `points`); exact, ties by smaller index
    NeighborGraph(idx, num_points)       the reverse adjacency of an index table (.idx, .offsets, .edges): build once per graph
    neighbor_gather(x, idx_or_graph)     -> x[idx] as (Q, K, C), zeros where idx is -1; differentiable w.r.t. x

    d2, idx = knn(pc._xyz, 16)                       # every few hundred steps
    graph = NeighborGraph(idx, pc._xyz.shape[0])     # with it
    nb = neighbor_gather(pc._xyz, graph)             # every step: (P, 16, 3), gradient to pc._xyz
    d2 = ((pc._xyz[:, None, :] - nb) ** 2).sum(-1)   # the differentiable squared distances

Every element of the gradient has one owner that adds its edges in ascending edge order: no atomics, the same bits every run, and
the bits of the sequential float32 sum in that order -- a contract, where the order in which `x[idx.long()]` accumulates under
autograd is an implementation detail of the framework.  The grouping of the edges by target is done once per graph and not on every
backward (tools/knn_bench.py: 3 to 10 times the speed of the indexing expression, forward plus backward).  HIP tensors only (no CPU
fallback).
"""
import ctypes
import functools

import torch

from diff_gaussian_rasterization import _C, _binding

MAX_K = 32   # include/gsr_knn.h GSR_KNN_MAX_K


_i, _vp = ctypes.c_int, ctypes.c_void_p
_lib, _run = _binding.declare("gsr_knn.h", {
    "gsr_knn_search_scratch_bytes": (ctypes.c_size_t, [_i, _i]),
    "gsr_knn_search": (_i, [_i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "gsr_knn_graph_scratch_bytes": (ctypes.c_size_t, [_i, _i]),
    "gsr_knn_graph_build": (_i, [_i, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "gsr_knn_gather": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "gsr_knn_gather_backward": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp]),
})
_check_device = functools.partial(_binding.check_device, "neighbour-graph kernels")


def _check_cloud(name, t):
    """A (rows, 3) float32 tensor, any strides -> rows"""
    _binding.check_matrix(name, t, "dimensions (rows, 3)", 3)
    return int(t.shape[0])


def _check_idx(idx, num_points, check):
    """An index table (Q, K) int32 with values in [-1, num_points); the values are looked at only on request (a read-back) -> (Q, K)"""
    if not torch.is_tensor(idx):
        raise TypeError("idx must be a tensor")
    if idx.dim() != 2:
        raise RuntimeError(f"idx must have dimensions (Q, K); got {tuple(idx.shape)}")
    if idx.dtype != torch.int32:
        raise RuntimeError(f"idx must be int32; got {idx.dtype}")
    if isinstance(num_points, bool) or not isinstance(num_points, int):
        raise TypeError(f"num_points must be an int, got {num_points!r}")
    if num_points < 0:
        raise ValueError(f"num_points must not be negative; got {num_points}")
    if idx.numel() >= 2 ** 31:
        raise RuntimeError(f"idx holds {idx.numel()} entries; the kernels index edges with 31 bits")
    if check and idx.numel():
        lo, hi = int(idx.min()), int(idx.max())
        if lo < -1 or hi >= num_points:
            raise ValueError(f"idx must hold values in [-1, {num_points}); found {lo} .. {hi}")
    return int(idx.shape[0]), int(idx.shape[1])


@torch.no_grad()
def knn(points, K, queries=None):
    """The K nearest points of every query -> (dist2 (Q, K) float32, idx (Q, K) int32).
    points (P, 3) float32.  queries (Q, 3) float32, or None: the queries are the points, and a point is left out of its own list by
    position, not by value (coincident points count with distance 0, as in distCUDA2).  With queries given nothing is left out.
    The distance is dx*dx + dy*dy + dz*dz in float32, left to right and uncontracted, as distCUDA2 forms it: ((d0 + d1) + d2) / 3 of
    knn(points, 3) has distCUDA2's bits.  Rows are ascending in (distance, index): among equal distances the smaller index comes
    first, so the result is unique.  Places without a neighbour (fewer than K candidates) hold +inf and -1.  1 <= K <= 32.
    Inputs are detached and may have any strides; the work runs on the tensors' device and the current stream."""
    P = _check_cloud("points", points)
    Q = P if queries is None else _check_cloud("queries", queries)
    _binding.check_int("K", K, 1, MAX_K)
    dev = _check_device(*((points,) if queries is None else (points, queries)))
    if Q * K >= 2 ** 31:
        raise RuntimeError(f"Q * K = {Q * K} entries; the kernels index them with 31 bits")
    lib = _lib()
    with torch.cuda.device(dev):
        if P == 0 or Q == 0:   # nobody to find
            return (torch.full((Q, K), float("inf"), dtype=torch.float32, device=dev), torch.full((Q, K), -1, dtype=torch.int32, device=dev))
        pts = points.detach().contiguous()
        qs = None if queries is None else queries.detach().contiguous()
        dist2 = torch.empty((Q, K), dtype=torch.float32, device=dev)
        idx = torch.empty((Q, K), dtype=torch.int32, device=dev)
        scratch = torch.empty((lib.gsr_knn_search_scratch_bytes(P, 0 if qs is None else Q),), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        _run("gsr_knn_search", P, pts.data_ptr(), Q, None if qs is None else qs.data_ptr(), K, dist2.data_ptr(), idx.data_ptr(), scratch.data_ptr(),
             stream.cuda_stream)
        for t in (scratch, pts) + (() if qs is None else (qs,)):
            t.record_stream(stream)
    return dist2, idx


class NeighborGraph:
    """The reverse adjacency of an index table idx (Q, K) int32 with values in [-1, num_points), -1 = no neighbour: edge e = q * K + k
    points at row idx[q, k].
        .idx      (Q, K) int32, contiguous
        .offsets  (num_points + 1,) int32
        .edges    (offsets[-1],) int32: the ids of the edges that have a target, those of target j at edges[offsets[j]:offsets[j+1]],
                  ascending inside a target (a stable sort of the edge ids by target); reading it waits for the device once
    Build it once per graph and hand it to neighbor_gather every step.  check=True reads the values of idx back and raises ValueError
    for one outside [-1, num_points); without it such a value is the caller's error."""

    def __init__(self, idx, num_points, check=False):
        Q, K = _check_idx(idx, num_points, check)
        dev = _check_device(idx)
        self.num_points = num_points
        self.idx = idx.detach().contiguous()
        E = Q * K
        lib = _lib()
        with torch.cuda.device(dev):
            self.offsets = torch.empty((num_points + 1,), dtype=torch.int32, device=dev)
            self._edges = torch.empty((E,), dtype=torch.int32, device=dev)
            scratch = torch.empty((lib.gsr_knn_graph_scratch_bytes(E, num_points),), dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev)
            _run("gsr_knn_graph_build", E, _C._ptr(self.idx), num_points, self.offsets.data_ptr(), _C._ptr(self._edges), None, _C._ptr(scratch),
                 stream.cuda_stream)
            scratch.record_stream(stream)
        self._num_valid = None

    @property
    def edges(self):
        if self._num_valid is None:
            self._num_valid = int(self.offsets[-1])
        return self._edges[:self._num_valid]


class _NeighborGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, graph):
        P = int(x.shape[0])
        Q, K = int(idx.shape[0]), int(idx.shape[1])
        C = x.numel() // P if P else int(torch.Size(x.shape[1:]).numel())
        dev = x.device
        with torch.cuda.device(dev):
            if P == 0 or Q * K == 0 or C == 0:
                out = torch.zeros((Q, K, C), dtype=torch.float32, device=dev)
            else:
                flat = x.detach().reshape(P, C).contiguous()
                out = torch.empty((Q, K, C), dtype=torch.float32, device=dev)
                _run("gsr_knn_gather", Q, K, C, flat.data_ptr(), idx.data_ptr(), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            if ctx.needs_input_grad[0] and graph is None:   # a bare idx: the graph is built here, and only when a gradient will flow
                graph = NeighborGraph(idx, P)
        ctx.graph, ctx.x_shape, ctx.C = graph, x.shape, C
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if grad_out is None or not ctx.needs_input_grad[0]:
            return None, None, None
        g, C = ctx.graph, ctx.C
        P = g.num_points
        dev = grad_out.device
        with torch.cuda.device(dev):
            if P == 0 or C == 0 or g._edges.numel() == 0:
                return torch.zeros(ctx.x_shape, dtype=torch.float32, device=dev), None, None
            go = grad_out.to(torch.float32).contiguous()
            gx = torch.empty((P, C), dtype=torch.float32, device=dev)
            _run("gsr_knn_gather_backward", P, C, g.offsets.data_ptr(), g._edges.data_ptr(), go.data_ptr(), gx.data_ptr(),
                 torch.cuda.current_stream(dev).cuda_stream)
        return gx.reshape(ctx.x_shape), None, None


def neighbor_gather(x, idx_or_graph, check=False):
    """x[idx] -> (Q, K, C) float32, zeros where idx is -1, differentiable w.r.t. x.
    x: any (P, ...) float32 tensor; its trailing dimensions are flattened to C.  idx_or_graph: a NeighborGraph over P points (build it
    once and reuse it), or a bare (Q, K) int32 index table, for which the graph is built on the fly, and only when x requires a
    gradient.  The differentiable squared distances of a search are then one line:
        d2 = ((queries[:, None, :] - neighbor_gather(points, idx)) ** 2).sum(-1)
    The gradient of x[j] is the float32 sum, started at 0, of the upstream rows of the edges that point at j in ascending edge order
    q * K + k: one owner per element, no atomics, the same bits every run.  check=True reads a bare idx back and raises ValueError for a
    value outside [-1, P)."""
    if not torch.is_tensor(x):
        raise TypeError("x must be a tensor")
    if x.dim() < 1:
        raise RuntimeError("x must have dimensions (P, ...); got a scalar")
    if x.dtype != torch.float32:
        raise RuntimeError(f"x must be float32; got {x.dtype}")
    P = int(x.shape[0])
    if isinstance(idx_or_graph, NeighborGraph):
        graph, idx = idx_or_graph, idx_or_graph.idx
        if graph.num_points != P:
            raise RuntimeError(f"the graph was built for {graph.num_points} points; x has {P} rows")
    else:
        graph, idx = None, idx_or_graph
        _check_idx(idx, P, check)
    _check_device(x, idx)
    return _NeighborGather.apply(x, idx.detach().contiguous(), graph)
