"""CPU: the neighbour graph (include/gsr_knn.h, fused_knn) without a device.  The numpy reference tests/torch_knn.py is pinned, not
trusted: its distances against scipy's cKDTree in float64, its K = 3 mean against the oracle of distCUDA2 bit for bit, its indices
against a float64 brute-force search wherever float64 can tell the neighbours apart; its graph and its backward against plain loops on
a hand example.  The C header compiles as C99, the library exports the six names and refuses bad arguments before any device work,
and the Python surface refuses what it must with no GPU present."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import torch_knn as tk
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsr_knn.h")
PKG = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd")
LIB = os.path.join(PKG, "libgsr_hip.so")
NAMES = ["gsr_knn_gather", "gsr_knn_gather_backward", "gsr_knn_graph_build", "gsr_knn_graph_scratch_bytes", "gsr_knn_search",
         "gsr_knn_search_scratch_bytes"]
KINDS = ["uniform", "clustered", "planar"]


# ---- the search reference is pinned ------------------------------------------------------------------------------------------------
def _float64_search(pts, n=33):
    """the n nearest others of every point by a float64 brute-force search -> (order (P, n), their squared distances), ascending in
    (distance, index)"""
    p64 = pts.astype(np.float64)
    d64 = np.zeros((len(pts), len(pts)))
    for a in range(3):
        d64 += (p64[None, :, a] - p64[:, None, a]) ** 2
    np.fill_diagonal(d64, np.inf)
    some = np.sort(np.argpartition(d64, n, axis=1)[:, :n + 1], axis=1)   # the n + 1 nearest, in index order
    o = np.argsort(np.take_along_axis(d64, some, axis=1), axis=1, kind="stable")[:, :n]
    order = np.take_along_axis(some, o, axis=1)
    return order, np.take_along_axis(d64, order, axis=1)


@pytest.fixture(scope="module")
def pinned():
    """(kind, P, K) -> (points, the reference's dist2 and idx, the float64 search's order and distances), computed once"""
    out = {}
    for P, Ks in ((3000, (3, 16)), (5000, (32,))):
        for kind in KINDS:
            pts = tk.cloud(P, 1, kind)
            order, near = _float64_search(pts)
            for K in Ks:
                out[kind, P, K] = (pts,) + tk.knn(pts, K) + (order, near)
    return out


CASES = [(P, K, kind) for P, K in ((3000, 3), (3000, 16), (5000, 32)) for kind in KINDS]


@pytest.mark.parametrize("P,K,kind", CASES)
def test_reference_distances_are_the_exact_nearest(pinned, P, K, kind):
    from scipy.spatial import cKDTree
    pts, d, i, _, _ = pinned[kind, P, K]
    p64 = pts.astype(np.float64)
    want = cKDTree(p64).query(p64, k=K + 1, workers=-1)[0][:, 1:] ** 2   # the point itself (distance 0) + K others
    err = np.abs(d.astype(np.float64) - want)
    print("worst relative distance error", float(np.max(err / (want + 1e-12))))
    assert d.dtype == np.float32 and i.dtype == np.int32 and d.shape == i.shape == (P, K)
    assert np.all(np.diff(d, axis=1) >= 0)
    assert np.all(err <= 1e-5 * want + 1e-9)


@pytest.mark.parametrize("kind", KINDS)
def test_reference_mean_of_three_is_the_oracle_of_distCUDA2(pinned, kind):
    pts, d, _, _, _ = pinned[kind, 3000, 3]
    np.testing.assert_array_equal(((d[:, 0] + d[:, 1]) + d[:, 2]) / np.float32(3.0), oracle.knn_mean_dist2(pts))


@pytest.mark.parametrize("P,K,kind", CASES)
def test_reference_indices_equal_a_float64_search_where_float64_can_tell(pinned, P, K, kind):
    """On every row whose consecutive float64 gaps, through the (K+1)-th neighbour, all exceed 4e-5 * d + 1e-9 -- four times the
    float32 bar of the distances, so that rounding cannot swap two neighbours -- the indices are those of the float64 search."""
    _, _, i, order, near = pinned[kind, P, K]
    order, near = order[:, :K + 1], near[:, :K + 1]
    kept = np.all(np.diff(near, axis=1) > 4e-5 * near[:, 1:] + 1e-9, axis=1)
    print("share of rows kept", float(kept.mean()))
    assert kept.mean() >= 0.90   # the condition: at most 10 % of the rows may be left out
    np.testing.assert_array_equal(i[kept], order[kept, :K].astype(np.int32))


def test_reference_edge_cases():
    pts = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 2, 0], [5, 5, 5]], np.float32)
    d, i = tk.knn(pts, 3)   # coincident points count with distance 0; ties by the smaller index
    np.testing.assert_array_equal(i[0], [1, 2, 3])
    np.testing.assert_array_equal(i[1], [0, 2, 3])
    np.testing.assert_array_equal(i[2], [0, 1, 3])
    np.testing.assert_array_equal(d[2], [1, 1, 5])
    d, i = tk.knn(pts[:3], 4)   # fewer than K others: +inf and -1
    np.testing.assert_array_equal(i, [[1, 2, -1, -1], [0, 2, -1, -1], [0, 1, -1, -1]])
    assert np.all(np.isinf(d[:, 2:])) and np.all(np.isfinite(d[:, :2]))
    d, i = tk.knn(pts, 2, queries=pts[:2])   # two sets: nothing is left out
    np.testing.assert_array_equal(i, [[0, 1], [0, 1]])
    np.testing.assert_array_equal(d, np.zeros((2, 2), np.float32))
    assert tk.knn(np.zeros((0, 3), np.float32), 3)[0].shape == (0, 3)
    d, i = tk.knn(np.zeros((0, 3), np.float32), 3, queries=pts)
    assert np.all(np.isinf(d)) and np.all(i == -1) and i.shape == (5, 3)


# ---- the graph and the backward references against plain loops -----------------------------------------------------------------
HAND_P = 7
HAND_IDX = np.array([[1, 2], [0, 2], [1, -1], [2, 6], [3, 5], [2, 0]], np.int32)   # a -1 entry; row 4 has in-degree 0


def test_graph_reference_on_a_hand_example():
    offsets, edges = tk.graph(HAND_IDX, HAND_P)
    rows = [[] for _ in range(HAND_P)]
    for e, j in enumerate(HAND_IDX.ravel().tolist()):
        if j >= 0:
            rows[j].append(e)
    assert rows[4] == [] and rows[2] == [1, 3, 6, 10]
    want_offsets, want_edges = [0], []
    for r in rows:
        want_edges += r
        want_offsets.append(len(want_edges))
    assert offsets.dtype == np.int32 and edges.dtype == np.int32
    assert offsets.tolist() == want_offsets and edges.tolist() == want_edges
    assert len(want_edges) == HAND_IDX.size - 1


def test_backward_reference_on_a_hand_example():
    C = 3
    g = (np.random.default_rng(3).normal(size=(HAND_IDX.shape[0], HAND_IDX.shape[1], C)) * 10.0 ** np.arange(C)).astype(np.float32)
    got = tk.gather_backward(g, HAND_IDX, HAND_P)
    want = np.zeros((HAND_P, C), np.float32)
    flat = g.reshape(-1, C)
    for e, j in enumerate(HAND_IDX.ravel().tolist()):   # ascending edge order
        if j >= 0:
            for c in range(C):
                want[j, c] = np.float32(want[j, c] + flat[e, c])
    np.testing.assert_array_equal(got, want)
    assert np.all(got[4] == 0)
    x = np.arange(HAND_P * C, dtype=np.float32).reshape(HAND_P, C) + 1
    out = tk.gather(x, HAND_IDX)
    assert np.all(out[2, 1] == 0) and np.array_equal(out[3, 1], x[6]) and np.array_equal(out[0, 0], x[1])


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def _lib():
    if not os.path.exists(LIB):
        __graft_entry__.build()
    from diff_gaussian_rasterization import _C
    return _C.lib()


def test_header_compiles_as_c99_and_refuses_before_any_device_work(tmp_path):
    """tests/cpp/knn_abi_check.c: the six symbols, every argument check (-1 with a text that names the function), zero counts with NULL
    pointers, scratch sizes 0 at 0 and growing with P, Q and E"""
    _lib()
    exe = tmp_path / "knn_abi_check"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "knn_abi_check.c"), "-o", str(exe), "-L" + PKG, "-lgsr_hip",
                        "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "knn_abi_check ok" in r.stdout, r.stdout + r.stderr


def test_the_library_exports_the_six_names():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr))) == NAMES
    L = _lib()
    for n in NAMES:
        assert hasattr(L, n), n
    # distCUDA2's entry points stay
    assert hasattr(L, "gsr_knn_mean_dist2") and hasattr(L, "gsr_knn_scratch_bytes")


# ---- the Python surface refuses before any kernel or library call ------------------------------------------------------------------
def test_python_refusals_without_a_device():
    import fused_knn as fk
    pts = torch.zeros((10, 3))
    idx = torch.zeros((10, 4), dtype=torch.int32)
    x = torch.zeros((10, 5))
    with pytest.raises(TypeError):
        fk.knn(pts.numpy(), 3)
    with pytest.raises(TypeError):
        fk.knn(pts, 3, queries=[[0.0, 0.0, 0.0]])
    with pytest.raises(TypeError):
        fk.knn(pts, 3.0)
    with pytest.raises(TypeError):
        fk.NeighborGraph(idx.numpy(), 10)
    with pytest.raises(TypeError):
        fk.neighbor_gather(x.numpy(), idx)
    with pytest.raises(TypeError):
        fk.neighbor_gather(x, idx.numpy())
    with pytest.raises(RuntimeError, match="no CPU path"):
        fk.knn(pts, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fk.knn(pts, 3, queries=pts)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fk.NeighborGraph(idx, 10)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fk.neighbor_gather(x, idx)
    with pytest.raises(RuntimeError, match="float32"):
        fk.knn(pts.double(), 3)
    with pytest.raises(RuntimeError, match="float32"):
        fk.knn(pts, 3, queries=pts.half())
    with pytest.raises(RuntimeError, match=r"\(rows, 3\)"):
        fk.knn(torch.zeros((10, 4)), 3)
    with pytest.raises(RuntimeError, match=r"\(rows, 3\)"):
        fk.knn(pts, 3, queries=torch.zeros((3,)))
    with pytest.raises(RuntimeError, match="int32"):
        fk.NeighborGraph(idx.long(), 10)
    with pytest.raises(RuntimeError, match=r"\(Q, K\)"):
        fk.NeighborGraph(idx.reshape(-1), 10)
    with pytest.raises(RuntimeError, match="float32"):
        fk.neighbor_gather(x.double(), idx)
    with pytest.raises(RuntimeError, match="int32"):
        fk.neighbor_gather(x, idx.long())
    with pytest.raises(RuntimeError, match="scalar"):
        fk.neighbor_gather(torch.zeros(()), idx)
    for K in (0, -1, 33):
        with pytest.raises(ValueError, match="1..32"):
            fk.knn(pts, K)
    bad = idx.clone()
    bad[3, 1] = 10
    with pytest.raises(ValueError, match=r"\[-1, 10\)"):
        fk.NeighborGraph(bad, 10, check=True)
    with pytest.raises(ValueError, match=r"\[-1, 10\)"):
        fk.neighbor_gather(x, bad, check=True)
    bad[3, 1] = -2
    with pytest.raises(ValueError, match=r"\[-1, 10\)"):
        fk.NeighborGraph(bad, 10, check=True)
    with pytest.raises(ValueError):
        fk.NeighborGraph(idx, -1)
    with pytest.raises(RuntimeError, match="no CPU path"):   # without the request the values are not looked at
        fk.NeighborGraph(bad, 10)
