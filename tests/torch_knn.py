"""numpy restatement of fused_knn (include/gsr_knn.h): the exact K-NN search, the reverse adjacency and the gather's backward, as
tests/test_knn_graph_cpu.py pins them and tests/test_knn_graph_gpu.py compares the kernels against, bit for bit.

search: brute force in float32 with the kernels' operation order (dx = c.x - q.x ..., then (dx*dx + dy*dy) + dz*dz), over chunks of
1000 queries; the self is masked by position; the rule (distance, index) is np.argsort(kind="stable") over columns in index order;
the padding is +inf and -1.  Only the columns at or below the row's K-th smallest distance go through the sort (np.partition finds
it), which leaves the result as it is and the cost at one pass over the distance matrix.
"""
import numpy as np


def cloud(P, seed, kind="uniform"):
    """the clouds of tests/test_knn.py"""
    r = np.random.default_rng(seed)
    if kind == "uniform":
        return r.uniform(-3, 3, size=(P, 3)).astype(np.float32)
    if kind == "clustered":   # COLMAP-like: dense surfaces + sparse outliers, spanning orders of magnitude in density
        c = r.normal(size=(max(P // 200, 1), 3)) * 4
        pts = c[r.integers(0, len(c), P)] + r.normal(size=(P, 3)) * r.choice([0.01, 0.1, 1.0], size=(P, 1))
        return pts.astype(np.float32)
    if kind == "planar":      # degenerate axis: z identical for all points, and x quantised (many exact ties)
        p = r.uniform(-1, 1, size=(P, 3)).astype(np.float32)
        p[:, 2] = 0.5
        p[:, 0] = np.round(p[:, 0] * 16) / 16
        return p
    raise ValueError(kind)


def dist2(q, pts):
    """(n, 3), (P, 3) float32 -> (n, P) float32 in the kernels' operation order"""
    dx = pts[None, :, 0] - q[:, None, 0]
    dy = pts[None, :, 1] - q[:, None, 1]
    dz = pts[None, :, 2] - q[:, None, 2]
    d = dx * dx
    d += dy * dy
    d += dz * dz
    assert d.dtype == np.float32
    return d


def knn(points, K, queries=None, chunk=1000):
    """-> (dist2 (Q, K) float32 ascending, idx (Q, K) int32); queries None: the points, each left out of its own list by position"""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    self_set = queries is None
    q = pts if self_set else np.ascontiguousarray(queries, dtype=np.float32)
    P, Q = pts.shape[0], q.shape[0]
    out_d = np.full((Q, K), np.inf, np.float32)
    out_i = np.full((Q, K), -1, np.int32)
    m = min(K, P - 1 if self_set else P)   # places that have a neighbour
    if m <= 0 or Q == 0:
        return out_d, out_i
    for lo in range(0, Q, chunk):
        rows = np.arange(lo, min(Q, lo + chunk))
        d = dist2(q[rows], pts)
        keep = np.ones(d.shape, bool)
        if self_set:
            keep[np.arange(len(rows)), rows] = False
        masked = np.where(keep, d, np.float32(np.inf))
        kth = np.partition(masked, m - 1, axis=1)[:, m - 1]
        cand = keep & (d <= kth[:, None])
        for r in range(len(rows)):
            cols = np.nonzero(cand[r])[0]                                  # index order
            order = cols[np.argsort(d[r, cols], kind="stable")[:m]]       # (distance, index)
            out_d[rows[r], :m] = d[r, order]
            out_i[rows[r], :m] = order
    return out_d, out_i


def graph(idx, P):
    """idx (Q, K) int32 in [-1, P) -> (offsets (P + 1,) int32, edges (E_valid,) int32): the edge ids q*K + k that have a target, grouped
    by target and ascending inside one"""
    flat = np.asarray(idx, np.int32).ravel()
    ids = np.nonzero(flat >= 0)[0]
    targets = flat[ids]
    edges = ids[np.argsort(targets, kind="stable")].astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(targets, minlength=P))]).astype(np.int32)
    return offsets, edges


def gather(x, idx):
    """x (P, C) float32, idx (Q, K) -> (Q, K, C) with zeros where idx is -1"""
    x = np.asarray(x, np.float32)
    out = x[np.maximum(idx, 0)]
    out[idx < 0] = 0
    return out


def gather_backward(grad_out, idx, P):
    """grad_out (Q, K, C) float32 -> grad_x (P, C) float32: np.add.at over the valid edges in ascending edge order on a float32 zero
    array -- sequential, unbuffered additions, so every row is the sequential float32 sum of its edges in that order"""
    g = np.asarray(grad_out, np.float32)
    C = g.shape[-1]
    g = g.reshape(-1, C)
    flat = np.asarray(idx, np.int32).ravel()
    ids = np.nonzero(flat >= 0)[0]
    out = np.zeros((P, C), np.float32)
    np.add.at(out, flat[ids], g[ids])
    return out
