"""Vector quantisation of the optimiser's leaves as fused HIP kernels (include/gsr_vq.h): the nearest-code search and the centroid
update that Compact3D, LightGaussian, "Compressed 3D Gaussian Splatting" and the codebook viewer formats start from.

    assign(x, codebook)                  -> (idx (N,) int32, dist2 (N,) float32); ties by smaller index, -1 / NaN for a row without a score
    update(x, idx, codebook, weight)     -> (codebook_new (K, D), count (K,) int32, wsum (K,) float32); the weighted mean of each code's rows
    kmeans(x, K, iters, init, weight)    -> (codebook (K, D), idx (N,), inertia (iters,) float64); Lloyd's algorithm on the two above
    lookup(codebook, idx)                -> codebook[idx], differentiable w.r.t. the codebook (fused_knn.neighbor_gather's fixed-order backward)
    quantize_gaussians(params, K, ...)   -> VQGaussians: named leaves as (codebook, idx), the others dense; .dequantize() .save() .load()

    vq = quantize_gaussians(pc, {"features_rest": 4096, "scaling": 4096, "rotation": 4096}, importance=weight_sum)
    vq.save("model_vq.npz"); pc2 = VQGaussians.load("model_vq.npz", device="cuda").dequantize()

The search scores a row against a code with |c|^2 - 2 x.c as one float32 fmaf chain on the matrix cores; nothing of size N x K is
stored.  The update has one owner per (code, column) that adds the code's rows in ascending row order in double (lists of 512 rows
and more in up to sixteen parts fixed by their length): no atomics.  Every
result has the same bits every run.  HIP tensors only (no CPU fallback); the container and dequantize() are plain copies and work on
any device.
"""
import ctypes
import functools

import numpy as np
import torch

import fused_knn
from diff_gaussian_rasterization import _binding

MAX_D = 64      # include/gsr_vq.h GSR_VQ_MAX_D
MAX_K = 65536   # include/gsr_vq.h GSR_VQ_MAX_K
FORMAT_VERSION = 1
LEAVES = ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity")   # gsr_model.GaussianParams, in its order


_i, _vp = ctypes.c_int, ctypes.c_void_p
_lib, _run = _binding.declare("gsr_vq.h", {   # update() groups the rows by code with fused_knn.NeighborGraph, through its table
    "gsr_vq_assign_scratch_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "gsr_vq_assign": (_i, [_i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "gsr_vq_update": (_i, [_i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
}, needs=("gsr_knn.h",))
_check_device = functools.partial(_binding.check_device, "quantisation kernels")
_check_int = _binding.check_int   # (name, v, least)


def _check_matrix(name, t, cols=None):
    """A (rows, D) float32 tensor, any strides -> (rows, D)"""
    _binding.check_matrix(name, t, "dimensions (rows, D)")
    if cols is not None and t.shape[1] != cols:
        raise RuntimeError(f"{name} must have {cols} columns as x has; got {tuple(t.shape)}")
    if not 1 <= t.shape[1] <= MAX_D:
        raise ValueError(f"{name} must have 1..{MAX_D} columns; got {t.shape[1]}")
    return int(t.shape[0]), int(t.shape[1])


def _check_codebook(codebook, D):
    K, _ = _check_matrix("codebook", codebook, D)
    if not 1 <= K <= MAX_K:
        raise ValueError(f"codebook must have 1..{MAX_K} rows; got {K}")
    return K


def _check_rows(name, t, N, dtype):
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a tensor")
    if t.dim() != 1 or t.shape[0] != N:
        raise RuntimeError(f"{name} must have dimensions ({N},); got {tuple(t.shape)}")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {str(dtype).replace('torch.', '')}; got {t.dtype}")


@torch.no_grad()
def assign(x, codebook):
    """The nearest code of every row -> (idx (N,) int32, dist2 (N,) float32).
    x (N, D) float32, codebook (K, D) float32, 1 <= D <= 64, 1 <= K <= 65536.  A code's score is the float32 chain
    fmaf(-2 x_k, c_k, acc) over k ascending, started at the chain fmaf(c_k, c_k, acc) from 0 (include/gsr_vq.h); idx is the smallest
    index among the codes of smallest score, -1 for a row whose every score is NaN or +inf.  dist2 is the squared distance to the
    chosen code evaluated in double from the differences and rounded once (NaN where idx is -1).  Inputs are detached and may have
    any strides; the work runs on the tensors' device and the current stream."""
    N, D = _check_matrix("x", x)
    K = _check_codebook(codebook, D)
    dev = _check_device(x, codebook)
    lib = _lib()
    with torch.cuda.device(dev):
        idx = torch.empty((N,), dtype=torch.int32, device=dev)
        dist2 = torch.empty((N,), dtype=torch.float32, device=dev)
        if N == 0:
            return idx, dist2
        xs, cb = x.detach().contiguous(), codebook.detach().contiguous()
        scratch = torch.empty((lib.gsr_vq_assign_scratch_bytes(N, D, K),), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        _run("gsr_vq_assign", N, D, xs.data_ptr(), K, cb.data_ptr(), idx.data_ptr(), dist2.data_ptr(), scratch.data_ptr(), stream.cuda_stream)
        for t in (scratch, xs, cb):
            t.record_stream(stream)
    return idx, dist2


@torch.no_grad()
def update(x, idx, codebook, weight=None):
    """Every code moves to the weighted mean of its rows -> (codebook_new (K, D) float32, count (K,) int32, wsum (K,) float32).
    idx (N,) int32 with values in [-1, K), -1 = the row belongs to no code (a value outside counts as -1); weight (N,) float32 >= 0
    or None = 1.  Sums are formed in double, the rows of a code added in ascending row order (include/gsr_vq.h: the split of long
    lists depends on their length alone), and rounded once after the division.
    A code without rows, or whose weights add up to 0, keeps its bits; count tells the caller which to re-seed."""
    N, D = _check_matrix("x", x)
    K = _check_codebook(codebook, D)
    _check_rows("idx", idx, N, torch.int32)
    if weight is not None:
        _check_rows("weight", weight, N, torch.float32)
    dev = _check_device(*((x, idx, codebook) + (() if weight is None else (weight,))))
    with torch.cuda.device(dev):
        out = codebook.detach().clone(memory_format=torch.contiguous_format)
        count = torch.zeros((K,), dtype=torch.int32, device=dev)
        wsum = torch.zeros((K,), dtype=torch.float32, device=dev)
        if N == 0:
            return out, count, wsum
        graph = fused_knn.NeighborGraph(idx[:, None], K)   # each code's rows, ascending: a stable sort of the row ids by code
        xs = x.detach().contiguous()
        w = None if weight is None else weight.detach().contiguous()
        stream = torch.cuda.current_stream(dev)
        _run("gsr_vq_update", N, D, xs.data_ptr(), None if w is None else w.data_ptr(), K, graph.offsets.data_ptr(), graph._edges.data_ptr(),
             out.data_ptr(), count.data_ptr(), wsum.data_ptr(), stream.cuda_stream)
        for t in (xs,) + (() if w is None else (w,)):
            t.record_stream(stream)
    return out, count, wsum


def _weighted_mean(x, weight):
    """The weighted column mean, formed in double and rounded once -> (D,) float32"""
    S = torch.zeros((x.shape[1],), dtype=torch.float64, device=x.device)
    W = torch.zeros((), dtype=torch.float64, device=x.device)
    for lo in range(0, x.shape[0], 1 << 20):   # bounds the double copies
        xd = x[lo:lo + (1 << 20)].double()
        if weight is None:
            S += xd.sum(0)
            W += xd.shape[0]
        else:
            wd = weight[lo:lo + (1 << 20)].double()
            S += (wd[:, None] * xd).sum(0)
            W += wd.sum()
    return (S / W).float() if float(W) > 0 else torch.zeros_like(S, dtype=torch.float32)


@torch.no_grad()
def kmeans(x, K, iters=10, init=None, weight=None, seed=0, center=True):
    """Lloyd's algorithm -> (codebook (K, D) float32, idx (N,) int32, inertia (iters,) float64).
    init: a (K, D) tensor, or None = K distinct rows of x drawn with torch.Generator().manual_seed(seed).  weight: a per-row importance
    >= 0 (for a Gaussian model the weight_sum of contrib_stats accumulated over the training views), or None.  center=True
    subtracts the weighted column mean (formed in double, rounded once) from the rows and from init before the search and adds it back
    to the codebook: the expanded score |c|^2 - 2 x.c loses |mean|^2 / spread^2 digits otherwise.  Iteration t assigns against the
    current codebook, records inertia[t] = sum_i w_i dist2_i (summed in double) and moves the codes; idx is the last iteration's
    assignment and the codebook the means of exactly those rows.  A code that loses all its rows stays where it is (update()'s count
    tells which); re-seeding is the caller's policy."""
    N, D = _check_matrix("x", x)
    _check_int("K", K, 1)
    if K > MAX_K:
        raise ValueError(f"K must lie in 1..{MAX_K}; got {K}")
    _check_int("iters", iters, 1)
    if weight is not None:
        _check_rows("weight", weight, N, torch.float32)
    if init is not None:
        if _check_matrix("init", init, D)[0] != K:
            raise RuntimeError(f"init must have dimensions ({K}, {D}); got {tuple(init.shape)}")
    elif K > N:
        raise ValueError(f"K = {K} distinct rows cannot be drawn from {N}")
    dev = _check_device(*((x,) + (() if weight is None else (weight,)) + (() if init is None else (init,))))
    with torch.cuda.device(dev):
        x = x.detach()
        if init is None:
            g = torch.Generator().manual_seed(seed)
            init = x[torch.randperm(N, generator=g)[:K].to(dev)]
        codebook = init.detach().contiguous()
        mean = None
        if center and N:
            mean = _weighted_mean(x, weight)
            x, codebook = x - mean, codebook - mean
        x = x.contiguous()
        inertia = torch.zeros((iters,), dtype=torch.float64, device=dev)
        idx = torch.full((N,), -1, dtype=torch.int32, device=dev)
        wd = None if weight is None else weight.double()
        for t in range(iters):
            idx, dist2 = assign(x, codebook)
            d = torch.nan_to_num(dist2.double(), nan=0.0) if N else dist2.double()   # a row without a code takes no part
            inertia[t] = d.sum() if wd is None else (wd * d).sum()
            codebook = update(x, idx, codebook, weight)[0]
        if mean is not None:
            codebook = codebook + mean
    return codebook, idx, inertia


def lookup(codebook, idx):
    """codebook[idx] -> (N, D) float32, zeros where idx is -1; differentiable w.r.t. the codebook, whose gradient row j is the
    float32 sum of the upstream rows of code j in ascending row order (fused_knn.neighbor_gather): the forward of quantisation-aware
    fine-tuning."""
    if not torch.is_tensor(idx) or idx.dim() != 1:
        raise RuntimeError("idx must be a tensor of dimensions (N,)")
    return fused_knn.neighbor_gather(codebook, idx[:, None])[:, 0]


class VQGaussians:
    """A Gaussian model with some leaves replaced by (codebook (K, D), idx (N,) int32) and the others dense.
        .coded   {leaf name: (codebook, idx)}      .dense   {leaf name: tensor}      .shapes  {leaf name: the leaf's trailing shape}
    dequantize() -> gsr_model.GaussianParams whose coded leaves are codebook[idx] bit for bit."""

    def __init__(self, coded, dense, shapes, max_sh_degree=3, active_sh_degree=None):
        if set(coded) & set(dense) or set(coded) | set(dense) != set(LEAVES):
            raise ValueError(f"coded and dense must hold each of {LEAVES} once")
        for name, (cb, idx) in coded.items():
            if cb.dim() != 2 or cb.dtype != torch.float32:
                raise RuntimeError(f"the codebook of {name} must be a (K, D) float32 tensor; got {tuple(cb.shape)} {cb.dtype}")
            if idx.dim() != 1 or idx.dtype != torch.int32:
                raise RuntimeError(f"the indices of {name} must be an (N,) int32 tensor; got {tuple(idx.shape)} {idx.dtype}")
        self.coded, self.dense = dict(coded), dict(dense)
        self.shapes = {k: tuple(v) for k, v in shapes.items()}
        self.max_sh_degree = max_sh_degree
        self.active_sh_degree = max_sh_degree if active_sh_degree is None else active_sh_degree

    def leaf(self, name):
        if name in self.dense:
            return self.dense[name]
        cb, idx = self.coded[name]
        return cb[idx.long()].reshape((idx.shape[0],) + self.shapes[name])   # a copy: no arithmetic

    def dequantize(self, requires_grad=False):
        import gsr_model
        mk = lambda t: t.detach().clone().requires_grad_(requires_grad)
        return gsr_model.GaussianParams(*[mk(self.leaf(n)) for n in LEAVES], self.max_sh_degree, self.active_sh_degree)

    def save(self, path):
        """An .npz (numpy, uncompressed): float32 codebooks and dense leaves, indices as uint16 where the codebook has at most 65536
        rows and int32 beyond, the trailing shapes and a format version."""
        out = {"format_version": np.int32(FORMAT_VERSION), "sh_degree": np.array([self.max_sh_degree, self.active_sh_degree], dtype=np.int32)}
        for name, t in self.dense.items():
            out["dense/" + name] = t.detach().cpu().numpy().astype(np.float32, copy=False)
        for name, (cb, idx) in self.coded.items():
            i = idx.detach().cpu().numpy()
            if i.size and (i.min() < 0 or i.max() >= cb.shape[0]):
                raise ValueError(f"the indices of {name} must lie in [0, {cb.shape[0]}); found {i.min()} .. {i.max()}")
            out["codebook/" + name] = cb.detach().cpu().numpy().astype(np.float32, copy=False)
            out["idx/" + name] = i.astype(np.uint16 if cb.shape[0] <= 65536 else np.int32)
            out["shape/" + name] = np.asarray(self.shapes[name], dtype=np.int64)
        with open(path, "wb") as f:
            np.savez(f, **out)

    @classmethod
    def load(cls, path, device=None):
        with np.load(path, allow_pickle=False) as z:
            version = int(z["format_version"])
            if version != FORMAT_VERSION:
                raise ValueError(f"{path}: format version {version}; this reader knows {FORMAT_VERSION}")
            mk = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            dense = {k[6:]: mk(z[k]) for k in z.files if k.startswith("dense/")}
            coded = {k[9:]: (mk(z[k]), mk(z["idx/" + k[9:]].astype(np.int32))) for k in z.files if k.startswith("codebook/")}
            shapes = {k[6:]: tuple(int(v) for v in z[k]) for k in z.files if k.startswith("shape/")}
            deg = z["sh_degree"]
            return cls(coded, dense, shapes, int(deg[0]), int(deg[1]))


_DEFAULT_K = {"features_rest": 4096, "scaling": 4096, "rotation": 4096}


@torch.no_grad()
def quantize_gaussians(params, K=None, importance=None, iters=10, seed=0):
    """A gsr_model.GaussianParams -> VQGaussians.  K: {leaf name: codebook size}, default features_rest, scaling and rotation at 4096
    (a size above the number of Gaussians is cut to it).  Each named leaf is flattened to (N, D), D <= 64, clustered with kmeans
    (importance = the per-Gaussian weight, e.g. contrib_stats' weight_sum summed over the training views) and replaced by the codebook
    and each row's nearest code.  Rotations are normalised before clustering and the codebook rows once more after it, so that a
    dequantised rotation is a unit quaternion; the indices are assigned against the final codebook.  Every other leaf stays dense."""
    K = dict(_DEFAULT_K if K is None else K)
    for name in K:
        if name not in LEAVES:
            raise ValueError(f"K names the leaf {name!r}; the leaves are {LEAVES}")
    leaves = dict(zip(LEAVES, (p.detach() for p in params.parameters())))
    N = int(leaves["xyz"].shape[0])
    coded, dense, shapes = {}, {}, {}
    for name in LEAVES:
        t = leaves[name]
        if name not in K:
            dense[name] = t.clone()
            continue
        rows = t.reshape(N, -1).float()
        if name == "rotation":
            rows = torch.nn.functional.normalize(rows)
        k = min(int(K[name]), N)
        cb, _, _ = kmeans(rows, k, iters=iters, weight=importance, seed=seed)
        if name == "rotation":
            cb = torch.nn.functional.normalize(cb)
        idx, _ = assign(rows, cb)
        if int(idx.min()) < 0:
            raise ValueError(f"the leaf {name} holds rows that are not finite")
        coded[name], shapes[name] = (cb, idx), tuple(t.shape[1:])
    return VQGaussians(coded, dense, shapes, params.max_sh_degree, params.active_sh_degree)
