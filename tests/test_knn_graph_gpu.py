"""GPU: fused_knn (include/gsr_knn.h) against the numpy reference tests/torch_knn.py, which tests/test_knn_graph_cpu.py pins.  Every
comparison is array_equal and nothing is left out: the search is exact and ordered by (distance, index), the graph is a stable sort,
the gather's backward is the sequential float32 sum in ascending edge order."""
import functools

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import torch_knn as tk

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _ref32(kind, P, seed):
    """the reference search of a cloud at K = 32, computed once: a smaller K is its first K columns (the order is total)"""
    pts = tk.cloud(P, seed, kind)
    d, i = tk.knn(pts, 32)
    return pts, d, i


def _assert_search(got, want):
    d, i = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert d.dtype == np.float32 and i.dtype == np.int32
    np.testing.assert_array_equal(i, want[1])
    np.testing.assert_array_equal(d, want[0])


# ---- search, self-set --------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 3, 4, 5, 33, 63, 64, 65, 255, 256, 257, 4096, 4097]   # fewer than K neighbours, the wave, box and super-box seams
KS = [1, 3, 4, 5, 8, 16, 20, 32]


@pytest.mark.parametrize("P", SIZES)
def test_self_search_at_every_seam_and_K(P):
    _need_gpu()
    from fused_knn import knn
    pts, d, i = _ref32("uniform", P, 7)
    t = _dev(pts)
    for K in KS:
        _assert_search(knn(t, K), (d[:, :K], i[:, :K]))


@pytest.mark.parametrize("kind,P,K", [("planar", 5000, 16), ("clustered", 20000, 16), ("uniform", 20011, 32)])
def test_self_search_on_the_clouds(kind, P, K):
    """planar: a degenerate axis and a quantised x (exact ties, where they occur, are decided by the index rule; the coincident and
    the doubled cloud below are all ties)"""
    _need_gpu()
    from fused_knn import knn
    pts, d, i = _ref32(kind, P, 7)
    _assert_search(knn(_dev(pts), K), (d[:, :K], i[:, :K]))


def test_coincident_points():
    _need_gpu()
    from fused_knn import knn
    pts = np.full((300, 3), 0.25, np.float32)
    d, i = knn(_dev(pts), 5)
    want = np.array([[j for j in range(6) if j != r][:5] for r in range(300)], np.int32)   # the five smallest other than the row
    np.testing.assert_array_equal(i.cpu().numpy(), want)
    np.testing.assert_array_equal(d.cpu().numpy(), np.zeros((300, 5), np.float32))


def test_a_cloud_concatenated_with_itself():
    _need_gpu()
    from fused_knn import knn
    half = tk.cloud(2000, 5, "uniform")
    pts = np.concatenate([half, half])
    want = tk.knn(pts, 3)
    assert np.all(want[0][:, 0] == 0)
    _assert_search(knn(_dev(pts), 3), want)


@pytest.mark.parametrize("kind,P", [("planar", 5000), ("clustered", 20000)])
def test_three_nearest_tie_to_distCUDA2(kind, P):
    _need_gpu()
    from fused_knn import knn
    from simple_knn._C import distCUDA2
    t = _dev(tk.cloud(P, 7, kind))
    d = knn(t, 3)[0].cpu().numpy()   # on the host: torch divides by a scalar through its reciprocal, which is not the kernel's division
    np.testing.assert_array_equal(((d[:, 0] + d[:, 1]) + d[:, 2]) / np.float32(3.0), distCUDA2(t).cpu().numpy())


# ---- search, two-set ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,P", [(1, 257), (65, 5000), (300, 257), (5000, 300)])
def test_two_set_search(Q, P):
    _need_gpu()
    from fused_knn import knn
    pts = tk.cloud(P, 11, "clustered")
    q = tk.cloud(Q, 12, "uniform")
    q[::3] = pts[np.arange(0, Q, 3) % P]   # queries equal to reference points: they are not left out
    for K in (1, 5, 16, 32):
        want = tk.knn(pts, K, queries=q)
        assert np.all(want[0][::3, 0] == 0)
        _assert_search(knn(_dev(pts), K, queries=_dev(q)), want)


def test_two_set_queries_far_outside_the_reference_bounds():
    _need_gpu()
    from fused_knn import knn
    pts = tk.cloud(3000, 13, "uniform")           # extent 6 on every axis
    q = tk.cloud(400, 14, "uniform")
    q[:, 0] += np.linspace(0, 600, 400, dtype=np.float32)   # up to 100 x the extent away on one axis
    q[::2, 1] -= 50
    want = tk.knn(pts, 8, queries=q)
    _assert_search(knn(_dev(pts), 8, queries=_dev(q)), want)


def test_two_set_with_fewer_points_than_K_and_empty_sets():
    _need_gpu()
    from fused_knn import knn
    pts, q = tk.cloud(5, 15, "uniform"), tk.cloud(70, 16, "uniform")
    want = tk.knn(pts, 8, queries=q)
    assert np.all(want[1][:, 5:] == -1) and np.all(np.isinf(want[0][:, 5:]))
    _assert_search(knn(_dev(pts), 8, queries=_dev(q)), want)
    empty = torch.zeros((0, 3), device="cuda")
    d, i = knn(_dev(pts), 4, queries=empty)           # Q = 0
    assert d.shape == (0, 4) and i.shape == (0, 4) and d.dtype == torch.float32 and i.dtype == torch.int32
    _assert_search(knn(empty, 4, queries=_dev(q)), tk.knn(np.zeros((0, 3), np.float32), 4, queries=q))   # P = 0
    d, i = knn(empty, 4)
    assert d.shape == (0, 4) and i.shape == (0, 4)


def test_strided_input_and_repeatability():
    _need_gpu()
    from fused_knn import knn
    pts, d, i = _ref32("clustered", 20000, 7)
    wide = torch.zeros((20000, 2, 5), device="cuda")
    wide[:, 1, 1:4] = _dev(pts)
    view = wide[:, 1, 1:4]
    assert not view.is_contiguous()
    a = knn(view, 16)
    b = knn(view.contiguous(), 16)
    c = knn(view, 16)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    _assert_search(a, (d[:, :16], i[:, :16]))
    q = wide[:300, 1, 1:4]
    assert torch.equal(knn(view, 4, queries=q)[1], knn(view, 4, queries=q.contiguous())[1])


# ---- graph -------------------------------------------------------------------------------------------------------------------------
def _graph_cases():
    r = np.random.default_rng(21)
    cases = {}
    cases["search_clustered"] = (_ref32("clustered", 20000, 7)[2][:, :16], 20000)
    cases["search_short"] = (_ref32("uniform", 5, 7)[2][:, :8], 5)                 # -1 entries: fewer than K neighbours
    cases["two_set"] = (tk.knn(tk.cloud(300, 11, "clustered"), 5, queries=tk.cloud(5000, 12, "uniform"))[1], 300)
    cases["empty"] = (np.zeros((0, 4), np.int32), 10)                              # E = 0
    cases["K1"] = (r.integers(0, 700, size=(1000, 1)).astype(np.int32), 700)
    cases["one_target"] = (np.zeros((1250, 4), np.int32), 1)                       # P = 1 with 5000 edges, all on one target
    idx = r.integers(-1, 400, size=(3000, 6)).astype(np.int32)                     # -1 entries ...
    idx[idx % 7 == 3] = 0                                                          # ... and targets with in-degree 0
    cases["holes"] = (idx, 400)
    for P in (255, 256, 257):
        cases[f"rows{P}"] = (r.integers(-1, P, size=(P, 3)).astype(np.int32), P)
    return cases


GRAPH_CASES = ["search_clustered", "search_short", "two_set", "empty", "K1", "one_target", "holes", "rows255", "rows256", "rows257"]


@functools.lru_cache(maxsize=None)
def _cases():
    return _graph_cases()


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_graph_is_the_stable_sort_of_the_edges_by_target(name):
    _need_gpu()
    from fused_knn import NeighborGraph
    idx, P = _cases()[name]
    offsets, edges = tk.graph(idx, P)
    g = NeighborGraph(_dev(idx), P, check=True)
    assert g.offsets.dtype == torch.int32 and g.edges.dtype == torch.int32
    np.testing.assert_array_equal(g.offsets.cpu().numpy(), offsets)
    np.testing.assert_array_equal(g.edges.cpu().numpy(), edges)
    np.testing.assert_array_equal(g.idx.cpu().numpy(), idx)
    if name == "holes":
        assert np.any(np.diff(offsets) == 0) and np.any(idx == -1)
    again = NeighborGraph(_dev(idx), P)
    assert torch.equal(again.offsets, g.offsets) and torch.equal(again.edges, g.edges)


# ---- gather and its backward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 4, 48, 65])   # 65 channels go beyond a wave
@pytest.mark.parametrize("name", ["search_short", "one_target", "holes", "rows257"])
def test_gather_and_its_backward(name, C):
    _need_gpu()
    from fused_knn import NeighborGraph, neighbor_gather
    idx, P = _cases()[name]
    r = np.random.default_rng(C)
    x = r.normal(size=(P, C)).astype(np.float32)
    go = (r.normal(size=idx.shape + (C,)) * 10.0 ** r.integers(-3, 4, size=idx.shape + (1,))).astype(np.float32)
    t = _dev(x).requires_grad_(True)
    g = NeighborGraph(_dev(idx), P)
    out = neighbor_gather(t, g)
    np.testing.assert_array_equal(out.detach().cpu().numpy(), tk.gather(x, idx))
    out.backward(_dev(go))
    want = tk.gather_backward(go, idx, P)   # the one-target case: a 5000-term sequential sum per channel
    np.testing.assert_array_equal(t.grad.cpu().numpy(), want)
    first = t.grad.clone()
    t.grad = None
    neighbor_gather(t, g).backward(_dev(go))
    assert torch.equal(t.grad, first)


def test_gather_flattens_trailing_dimensions_and_skips_the_graph_without_a_gradient():
    _need_gpu()
    import fused_knn as fk
    idx, P = _cases()["holes"]
    x = np.random.default_rng(2).normal(size=(P, 2, 3)).astype(np.float32)
    built = []
    orig = fk.NeighborGraph.__init__
    try:
        fk.NeighborGraph.__init__ = lambda self, *a, **k: (built.append(1), orig(self, *a, **k))[1]
        out = fk.neighbor_gather(_dev(x), _dev(idx))          # no gradient asked for: no graph
        assert not built and not out.requires_grad
        np.testing.assert_array_equal(out.cpu().numpy(), tk.gather(x.reshape(P, 6), idx))
        t = _dev(x).requires_grad_(True)
        fk.neighbor_gather(t, _dev(idx)).sum().backward()
        assert built == [1] and t.grad.shape == (P, 2, 3)
    finally:
        fk.NeighborGraph.__init__ = orig
    counts = np.bincount(idx[idx >= 0], minlength=P).astype(np.float32)   # small integers: exact in any order
    np.testing.assert_array_equal(t.grad.cpu().numpy(), np.broadcast_to(counts[:, None, None], (P, 2, 3)))


# ---- autograd ----------------------------------------------------------------------------------------------------------------------
def test_autograd_loss_has_the_bits_of_the_reference_pieces():
    _need_gpu()
    from fused_knn import NeighborGraph, knn, neighbor_gather
    pts = tk.cloud(500, 31, "clustered")
    idx = tk.knn(pts, 8)[1]
    x = _dev(pts).requires_grad_(True)
    d2, got_idx = knn(x, 8)
    np.testing.assert_array_equal(got_idx.cpu().numpy(), idx)
    g = NeighborGraph(got_idx, 500)
    ((x[:, None] - neighbor_gather(x, g)) ** 2).sum().backward()
    with_graph = x.grad.clone()
    x.grad = None
    ((x[:, None] - neighbor_gather(x, got_idx)) ** 2).sum().backward()   # a bare idx
    assert torch.equal(x.grad, with_graph)
    # the same loss from the reference pieces: the gather's forward and backward are numpy's, the rest is the same torch graph
    nb = _dev(tk.gather(pts, idx)).requires_grad_(True)
    y = _dev(pts).requires_grad_(True)
    ((y[:, None] - nb) ** 2).sum().backward()
    through = _dev(tk.gather_backward(nb.grad.cpu().numpy(), idx, 500))
    assert torch.equal(with_graph, y.grad + through)
