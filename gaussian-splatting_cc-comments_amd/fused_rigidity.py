"""The neighbour-rigidity losses of Dynamic 3D Gaussians (Luiten et al., 3DV 2024: local rigidity, rotation similarity, isometry) as
fused HIP kernels over the neighbour graph of fused_knn (include/gsr_rigidity.h): the three terms, their weighted total and its
gradients with respect to the positions and the raw rotations from one pass over the edges and one fixed-order sum per point, where
the stock sequence is about forty elementwise launches over (P, K, 3) and (P, K, 4) intermediates that autograd keeps.

    RigidityState.capture(xyz, rotation, K=20, weight_lambda=2000.0, mask=None)     once per graph (per time step in the paper)
    RigidityState.from_tables(idx, prev_offset, prev_dist, weight, prev_inv_rot, num_points)
    rigidity_loss(xyz, rotation, state, rigid=4.0, rot=4.0, iso=2.0)      -> scalar, differentiable w.r.t. xyz and rotation
    rigidity_loss_terms(...)                                              -> (loss, rigid, rot, iso), the terms detached
    rigidity_loss_and_grads(...)                                          -> (values (4,), {"xyz": ..., "rotation": ...}), no autograd

    state = RigidityState.capture(pc._xyz, pc._rotation, K=20, mask=is_foreground)   # after a time step has converged
    loss = loss + rigidity_loss(pc._xyz, pc._rotation, state)                         # every step of the next one

For a valid edge (i, k), j = idx[i, k] >= 0, with q = r / |r|, rel = q (x) p (Hamilton product, (w, x, y, z)), R = build_rotation(rel)
and c = x_j - x_i:  rigid = sqrt(w |R^T c - o|^2 + 1e-20), rot = sqrt(w |rel_j - rel_i|^2 + 1e-20),
iso = sqrt(w (sqrt(|c|^2 + 1e-20) - d)^2 + 1e-20).  Every term is the sum over the valid edges divided by their number N_e -- the
paper's .mean() when the table has no -1 -- and 0 when there is no edge.  A zero quaternion gives unspecified values.
No atomics: every element of a gradient has one owner that adds its contributions in a fixed order, so every output has the same
bits in every run.  HIP tensors only (no CPU fallback); the leaves may have any strides.
"""
import ctypes

import torch

import fused_knn
from diff_gaussian_rasterization import _C, _binding
from fused_knn import MAX_K, NeighborGraph, _check_cloud, _check_device, _check_idx

GRADS = ("xyz", "rotation")
LANES = 8   # csrc/rigidity.hip GSR_RIG_LANES: the lanes that share a point's edges

_i, _f, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
_lib, _run = _binding.declare("gsr_rigidity.h", {   # the graph a state holds is built through fused_knn's table
    "gsr_rigidity_scratch_bytes": (ctypes.c_size_t, [_i, _i]),
    "gsr_rigidity_loss": (_i, [_i, _i] + [_vp] * 9 + [_f, _f, _f] + [_vp] * 5),
}, needs=("gsr_knn.h",))


def _check_table(name, t, shape, dtype=torch.float32):
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a tensor")
    if tuple(t.shape) != shape:
        raise RuntimeError(f"{name} must have dimensions {shape}; got {tuple(t.shape)}")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {str(dtype).replace('torch.', '')}; got {t.dtype}")


def _check_rotation(rotation, P):
    _binding.check_matrix("rotation", rotation, "dimensions (rows, 4)", 4)
    if rotation.shape[0] != P:
        raise RuntimeError(f"xyz has {P} rows; rotation has {rotation.shape[0]}")


def _check_K(K):
    _binding.check_int("K", K, 1, MAX_K)


def tables_from_search(xyz, rotation, dist2, ids, weight_lambda=2000.0, rows=None):
    """The captured tables from a search result, on whatever device the tensors live (plain tensor operations, once per graph).
    dist2, ids (n, K): the search over xyz[rows] (rows None: over all of xyz), ids indexing that subset.  -> idx (P, K) int32 into the
    full rows, all -1 on the rows that were not searched; prev_offset (P, K, 3) = x_j - x_i; prev_dist (P, K) = sqrt(dist2);
    weight (P, K) = exp(-weight_lambda dist2); prev_inv_rot (P, 4) = the conjugate of rotation / |rotation|.  Places with idx = -1
    hold zeros (the search's +inf distance never reaches an exp or a difference)."""
    P, K = int(xyz.shape[0]), int(ids.shape[1])
    dev = xyz.device
    if rows is None:
        idx, d2 = ids, dist2
    else:
        idx = torch.full((P, K), -1, dtype=torch.int32, device=dev)
        d2 = torch.zeros((P, K), dtype=torch.float32, device=dev)
        if rows.numel():
            idx[rows] = torch.where(ids >= 0, rows[ids.clamp(min=0).long()].to(torch.int32), ids)
            d2[rows] = dist2
    valid = idx >= 0
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    d2 = torch.where(valid, d2, zero)
    x = xyz.detach()
    prev_offset = torch.where(valid[..., None], x[idx.long().clamp(min=0)] - x[:, None], zero)
    weight = torch.where(valid, torch.exp(-float(weight_lambda) * d2), zero)
    r = rotation.detach()
    q = r / torch.sqrt((r * r).sum(-1, keepdim=True))
    prev_inv_rot = q * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=torch.float32, device=dev)
    return idx.contiguous(), prev_offset.contiguous(), torch.sqrt(d2), weight, prev_inv_rot.contiguous()


class RigidityState:
    """What the losses keep from the moment of capture, constants without a gradient:
        .idx (P, K) int32 in [-1, P)   .prev_offset (P, K, 3)   .prev_dist (P, K)   .weight (P, K)   .prev_inv_rot (P, 4)
        .graph        the NeighborGraph of idx (its reverse adjacency)
        .num_points   P        .K        .num_edges   N_e, the number of valid edges, read back once when the state is made
    The tables are kept in the paper's own (P, K, .) layout, which is the layout the kernels read.  Build a state with capture() or
    from_tables()."""

    def __init__(self, idx, prev_offset, prev_dist, weight, prev_inv_rot, num_points, check=False):
        Q, K = _check_idx(idx, num_points, check)
        if Q != num_points:
            raise RuntimeError(f"idx must have one row per point: {num_points} points, {Q} rows")
        if K > MAX_K:
            raise ValueError(f"K must lie in 1..{MAX_K}; got {K}")
        _check_table("prev_offset", prev_offset, (Q, K, 3))
        _check_table("prev_dist", prev_dist, (Q, K))
        _check_table("weight", weight, (Q, K))
        _check_table("prev_inv_rot", prev_inv_rot, (Q, 4))
        _check_device(idx, prev_offset, prev_dist, weight, prev_inv_rot)
        self.num_points, self.K = num_points, K
        self.graph = NeighborGraph(idx, num_points)
        self.idx = self.graph.idx
        self.prev_offset, self.prev_dist, self.weight, self.prev_inv_rot = (t.detach().contiguous() for t in (prev_offset, prev_dist, weight, prev_inv_rot))
        self.num_edges = int(self.graph.offsets[-1])

    @classmethod
    def from_tables(cls, idx, prev_offset, prev_dist, weight, prev_inv_rot, num_points, check=False):
        """For callers who hold the paper's own tables: neighbor_indices (P, K) as int32 with -1 for "no neighbour", prev_offset
        (P, K, 3), neighbor_dist (P, K), neighbor_weight (P, K), prev_inv_rot (P, 4).  What prev_offset, prev_dist and weight hold where
        idx is -1 is never read.  check=True reads idx back and raises ValueError for a value outside [-1, P)."""
        return cls(idx, prev_offset, prev_dist, weight, prev_inv_rot, num_points, check)

    @classmethod
    @torch.no_grad()
    def capture(cls, xyz, rotation, K=20, weight_lambda=2000.0, mask=None):
        """The state of the current (detached) leaves: the K nearest neighbours of every point (fused_knn.knn), prev_offset = x_j - x_i,
        prev_dist = sqrt(dist2), weight = exp(-weight_lambda dist2), prev_inv_rot = the conjugate of rotation / |rotation|.
        mask: a (P,) bool tensor; the search runs over the rows it selects only (the paper's foreground set) and its indices are mapped
        back to full rows; the other rows are all -1, contribute nothing and get zero gradients, so the leaves are never sliced."""
        P = _check_cloud("xyz", xyz)
        _check_rotation(rotation, P)
        _check_K(K)
        if isinstance(weight_lambda, bool) or not isinstance(weight_lambda, (int, float)):
            raise TypeError(f"weight_lambda must be a number, got {weight_lambda!r}")
        if mask is not None:
            _check_table("mask", mask, (P,), torch.bool)
        dev = _check_device(*((xyz, rotation) if mask is None else (xyz, rotation, mask)))
        with torch.cuda.device(dev):
            rows = None if mask is None else torch.nonzero(mask).flatten()
            dist2, ids = fused_knn.knn(xyz if rows is None else xyz.detach()[rows], K)
            return cls(*tables_from_search(xyz, rotation, dist2, ids, weight_lambda, rows), P)


def _check_call(xyz, rotation, state, weights):
    P = _check_cloud("xyz", xyz)
    _check_rotation(rotation, P)
    if not isinstance(state, RigidityState):
        raise TypeError(f"state must be a RigidityState, got {type(state).__name__}")
    if state.num_points != P:
        raise RuntimeError(f"the state was built for {state.num_points} points; xyz has {P} rows")
    for name, w in zip(("rigid", "rot", "iso"), weights):
        if isinstance(w, bool) or not isinstance(w, (int, float)):
            raise TypeError(f"{name} must be a number, got {w!r}")
    dev = _check_device(xyz, rotation)
    if state.idx.device != dev:
        raise RuntimeError(f"the state lives on {state.idx.device}; the leaves on {dev}")
    return P, dev


def rigidity_loss_and_grads(xyz, rotation, state, rigid=4.0, rot=4.0, iso=2.0, want=GRADS):
    """-> (values (4,) device tensor: total, rigid, rot, iso; {"xyz": dL/dxyz (P, 3), "rotation": dL/drotation (P, 4)}), raw and without
    autograd.  The dictionary holds the gradients of the total named in `want`, formed in the same pass as the values; with want=()
    no per-edge row is stored and the per-point sum is not launched."""
    for k in want:
        if k not in GRADS:
            raise ValueError(f"want: unknown gradient {k!r}; the choices are {GRADS}")
    P, dev = _check_call(xyz, rotation, state, (rigid, rot, iso))
    lib = _lib()
    K, g = state.K, state.graph
    with torch.cuda.device(dev):
        x, r = xyz.detach().contiguous(), rotation.detach().contiguous()
        values = torch.empty(4, dtype=torch.float32, device=dev)
        grads = {k: torch.empty_like(t) for k, t in zip(GRADS, (x, r)) if k in want}
        scratch = torch.empty(lib.gsr_rigidity_scratch_bytes(P, K), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        ptr = _C._ptr
        _run("gsr_rigidity_loss", P, K, ptr(x), ptr(r), ptr(state.idx), ptr(state.prev_offset), ptr(state.prev_dist), ptr(state.weight),
             ptr(state.prev_inv_rot), ptr(g.offsets), g._edges.data_ptr() if g._edges.numel() else None, float(rigid), float(rot), float(iso),
             values.data_ptr(), ptr(grads.get("xyz")), ptr(grads.get("rotation")), ptr(scratch), stream.cuda_stream)
        for t in (scratch, x, r):
            t.record_stream(stream)
    return values, grads


class _Rigidity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, rotation, state, rigid, rot, iso):
        want = tuple(n for n, need in zip(GRADS, ctx.needs_input_grad) if need)   # and no other gradient is computed
        values, grads = rigidity_loss_and_grads(xyz, rotation, state, rigid, rot, iso, want)
        ctx.want, ctx.shapes = want, (xyz.shape, rotation.shape)
        ctx.save_for_backward(*(grads[n] for n in want))
        terms = values[1:]
        ctx.mark_non_differentiable(terms)
        return values[0], terms

    @staticmethod
    def backward(ctx, g_total, _g_terms):
        grads = dict(zip(ctx.want, ctx.saved_tensors))
        return tuple(grads[n] * g_total if n in grads else None for n in GRADS) + (None, None, None, None)


def rigidity_loss(xyz, rotation, state, rigid=4.0, rot=4.0, iso=2.0):
    """rigid * L_rigid + rot * L_rot + iso * L_iso (the defaults are the paper's weights), a scalar tensor, differentiable w.r.t. xyz
    (P, 3) and the raw rotation (P, 4): value and gradients come from one pass over the edges; backward multiplies the saved gradients
    by the upstream scalar.  Only the gradients autograd needs are computed."""
    _check_call(xyz, rotation, state, (rigid, rot, iso))
    return _Rigidity.apply(xyz, rotation, state, float(rigid), float(rot), float(iso))[0]


def rigidity_loss_terms(xyz, rotation, state, rigid=4.0, rot=4.0, iso=2.0):
    """-> (loss, L_rigid, L_rot, L_iso): the loss as rigidity_loss returns it, the three unweighted terms detached, for logging"""
    _check_call(xyz, rotation, state, (rigid, rot, iso))
    loss, terms = _Rigidity.apply(xyz, rotation, state, float(rigid), float(rot), float(iso))
    return loss, terms[0], terms[1], terms[2]
