"""CPU: the neighbour-rigidity losses (include/gsr_rigidity.h, fused_rigidity) without a device.  The float64 reference
tests/torch_rigidity.py is pinned against itself: its closed-form per-edge gradients equal float64 autograd of the plain sequence to
1e-12 of the largest gradient, with holes in the table; its clouds keep the weights where they say something.  The C header compiles
as C99, the library exports the two names and refuses bad arguments before any device work; the Python surface refuses what it must
with no GPU present; the bookkeeping of capture (mask, holes) is checked on CPU tensors against the reference's own capture."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import torch_knn
import torch_rigidity as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsr_rigidity.h")
PKG = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd")
LIB = os.path.join(PKG, "libgsr_hip.so")
CLOUDS = ((63, 20), (257, 20), (1000, 20), (4097, 16))


def _case(P, K, holes):
    xyz0, rot0 = tr.make_cloud(P)
    t = tr.capture(xyz0, rot0, K)
    if holes:   # scattered places, one whole row and one whole column; what the tables hold there must not matter
        g = torch.Generator().manual_seed(P)
        gone = torch.rand(P, K, generator=g) < 0.15
        gone[P // 2] = True
        gone[:, K // 2] = True
        t["idx"][gone] = -1
        for name in ("prev_offset", "prev_dist", "weight"):
            t[name][gone] = float("nan")
    xyz, rot = tr.perturb(xyz0, rot0, tr.SIDES[P])
    return xyz, rot, t


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("holes", (False, True))
@pytest.mark.parametrize("P,K", CLOUDS)
def test_closed_form_gradients_equal_float64_autograd(P, K, holes):
    xyz, rot, t = _case(P, K, holes)
    values, gx, gr = tr.loss_and_grads(xyz, rot, t)
    ax, ar, Sx, Sr = tr.analytic_grads(xyz, rot, t)
    ex = float((ax - gx).abs().max() / gx.abs().max())
    er = float((ar - gr).abs().max() / gr.abs().max())
    print(f"P = {P}, K = {K}, holes = {holes}: values {values.tolist()}; closed form against autograd: xyz {ex:.2e}, rotation {er:.2e}")
    assert bool(torch.isfinite(values).all()) and float(values[1]) > 0 and float(values[2]) > 0 and float(values[3]) > 0
    assert ex <= 1e-12 and er <= 1e-12
    # the scale of a row bounds the row (a sum of norms against the norm of the sum)
    assert bool((gx.norm(dim=1) <= Sx * (1 + 1e-9)).all()) and bool((gr.norm(dim=1) <= Sr * (1 + 1e-9)).all())
    if holes:
        assert bool((gr[P // 2].abs() <= Sr[P // 2]).all())
        # weights other than the paper's
        v2, gx2, gr2 = tr.loss_and_grads(xyz, rot, t, lambdas=(0.5, 0.0, 3.0))
        ax2, ar2, _, _ = tr.analytic_grads(xyz, rot, t, lambdas=(0.5, 0.0, 3.0))
        assert float((ax2 - gx2).abs().max() / gx2.abs().max()) <= 1e-12 and float((ar2 - gr2).abs().max() / gr2.abs().max()) <= 1e-12
        assert abs(float(v2[0]) - (0.5 * float(v2[1]) + 3.0 * float(v2[3]))) <= 1e-15


def test_reference_without_an_edge_is_zero():
    xyz0, rot0 = tr.make_cloud(1, side=0.1)
    t = tr.capture(xyz0, rot0, 3)
    assert bool((t["idx"] == -1).all())
    values, gx, gr = tr.loss_and_grads(xyz0, rot0, t)
    ax, ar, Sx, Sr = tr.analytic_grads(xyz0, rot0, t)
    for z in (values, gx, gr, ax, ar, Sx, Sr):
        assert bool((z == 0).all())


@pytest.mark.parametrize("P,K", CLOUDS)
def test_clouds_keep_the_weights_where_they_say_something(P, K):
    """beyond a weight of about 1e-3 the term is the constant 1e-10 and a comparison would check nothing: at least 0.8 of the valid
    edges stay above it"""
    xyz0, rot0 = tr.make_cloud(P)
    t = tr.capture(xyz0, rot0, K)
    share = tr.strong_share(t)
    print(f"P = {P}, K = {K}: share of valid edges with weight >= 1e-3: {share:.4f}")
    assert bool((t["idx"] >= 0).all()) and share >= 0.8


# ---- capture's bookkeeping on CPU tensors ------------------------------------------------------------------------------------------
def _search(xyz0, K, rows=None):
    d2, ids = torch_knn.knn((xyz0 if rows is None else xyz0[rows]).numpy(), K)
    return torch.from_numpy(d2), torch.from_numpy(ids)


def test_tables_from_search_equal_the_reference_capture():
    import fused_rigidity as fr
    xyz0, rot0 = tr.make_cloud(257)
    want = tr.capture(xyz0, rot0, 20)
    got = fr.tables_from_search(xyz0, rot0 * 3.0, *_search(xyz0, 20))   # the rotation is normalised at capture
    for name, g in zip(("idx", "prev_offset", "prev_dist", "weight"), got):
        assert torch.equal(g, want[name]), name
    assert float((got[4] - want["prev_inv_rot"]).abs().max()) <= 2.0 ** -22
    assert got[0].dtype == torch.int32 and all(g.dtype == torch.float32 and g.is_contiguous() for g in got[1:])


def test_tables_from_search_with_a_mask_and_with_holes():
    import fused_rigidity as fr
    P, K = 63, 20
    xyz0, rot0 = tr.make_cloud(P)
    mask = torch.zeros(P, dtype=torch.bool)
    mask[torch.randperm(P, generator=torch.Generator().manual_seed(3))[:12]] = True   # fewer rows than K: every searched row has holes
    rows = torch.nonzero(mask).flatten()
    want = tr.capture(xyz0, rot0, K, mask=mask)
    idx, off, dist, weight, pinv = fr.tables_from_search(xyz0, rot0, *_search(xyz0, K, rows), rows=rows)
    for name, g in zip(("idx", "prev_offset", "prev_dist", "weight", "prev_inv_rot"), (idx, off, dist, weight, pinv)):
        assert torch.equal(g, want[name]), name
    assert bool((idx[~mask] == -1).all()) and bool((idx[mask][:, :11] >= 0).all()) and bool((idx[mask][:, 11:] == -1).all())
    assert bool(mask[idx[idx >= 0].long()].all())                      # every neighbour is a masked row, named by its full-row index
    assert not bool((idx == torch.arange(P)[:, None]).any())           # and never the row itself
    hole = idx < 0
    for t in (off, dist, weight):                                      # zeros, not the inf or NaN of the search's +inf distance
        assert bool(torch.isfinite(t).all()) and bool((t[hole] == 0).all())
    j = idx[mask][:, 0].long()
    assert torch.equal(off[mask][:, 0], xyz0[j] - xyz0[mask])
    assert torch.allclose(dist[mask][:, 0], off[mask][:, 0].double().norm(dim=-1).float(), rtol=2.0 ** -22, atol=0)
    # an empty mask: a table without an edge
    none = torch.zeros(P, dtype=torch.bool)
    e = torch.nonzero(none).flatten()
    idx0, off0, dist0, w0, _ = fr.tables_from_search(xyz0, rot0, torch.zeros((0, K)), torch.zeros((0, K), dtype=torch.int32), rows=e)
    assert bool((idx0 == -1).all()) and bool((off0 == 0).all()) and bool((dist0 == 0).all()) and bool((w0 == 0).all())


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def _lib():
    if not os.path.exists(LIB):
        __graft_entry__.build()
    L = ctypes.CDLL(LIB)
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.gsr_last_error.restype = ctypes.c_char_p
    L.gsr_rigidity_scratch_bytes.restype = ctypes.c_size_t
    L.gsr_rigidity_scratch_bytes.argtypes = [i, i]
    L.gsr_rigidity_loss.restype = i
    L.gsr_rigidity_loss.argtypes = [i, i] + [vp] * 9 + [f, f, f] + [vp] * 5
    return L


def test_header_compiles_as_c99_and_names_what_the_library_exports():
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", "-I" + os.path.join(ROOT, "include"), HDR],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr)))
    assert names == ["gsr_rigidity_loss", "gsr_rigidity_scratch_bytes"]
    L = _lib()
    for n in names:
        assert hasattr(L, n), n


def test_library_refuses_before_any_device_work():
    L = _lib()
    sb = L.gsr_rigidity_scratch_bytes
    assert sb(0, 20) == 0 and sb(1000, 0) == 0 and sb(-1, 20) == 0 and sb(1000, 33) == 0 and sb(2 ** 27, 16) == 0
    assert 0 < sb(1000, 20) < sb(100000, 20) < sb(100000, 32)
    assert sb(1000, 20) >= 28 * 1000 * 20 + 44 * 1000
    # never dereferenced: every call below is refused before any device work
    buf = (ctypes.c_char * 256)()
    base = ctypes.addressof(buf)
    a = base + (-base) % 16                     # 16-byte aligned
    ok = dict(P=4, K=3, xyz=a, rotation=a, idx=a, prev_offset=a, prev_dist=a, weight=a, prev_inv_rot=a, offsets=a, edges=a, w=(4.0, 4.0, 2.0),
              values=a, grad_xyz=a, grad_rot=a, scratch=a, stream=None)

    def call(**change):
        k = dict(ok, **change)
        return L.gsr_rigidity_loss(k["P"], k["K"], k["xyz"], k["rotation"], k["idx"], k["prev_offset"], k["prev_dist"], k["weight"], k["prev_inv_rot"],
                                   k["offsets"], k["edges"], *k["w"], k["values"], k["grad_xyz"], k["grad_rot"], k["scratch"], k["stream"])

    def refused(what, **change):
        rc = call(**change)
        text = L.gsr_last_error().decode()
        assert rc == -1 and text.startswith("gsr_rigidity_loss:"), (what, rc, text)
        return text

    assert "negative" in refused("a negative P", P=-1)
    assert "negative" in refused("a negative K", K=-1)
    assert "1..32" in refused("K = 33", K=33)
    assert "values" in refused("values NULL", values=None)
    assert "values" in refused("values NULL with nothing to do", values=None, P=0)
    assert "2^31" in refused("P K = 2^31", P=2 ** 27, K=16)
    assert "2^31" in refused("P K beyond 2^31", P=2 ** 31 - 1, K=32)
    for name in ("xyz", "rotation", "idx", "prev_offset", "prev_dist", "weight", "prev_inv_rot", "offsets", "scratch"):
        assert "NULL" in refused(name + " NULL", **{name: None})
    assert "edges" in refused("edges NULL with a gradient", edges=None)
    assert "edges" in refused("edges NULL with one gradient", edges=None, grad_xyz=None)
    assert "aligned" in refused("unaligned scratch", scratch=a + 4)
    assert "aligned" in refused("unaligned scratch", scratch=a + 8)


# ---- the Python surface refuses before any kernel or library call ------------------------------------------------------------------
def _stub_state(P, K=4):
    """a state as the checks see it (a real one needs a device)"""
    import fused_rigidity as fr
    s = object.__new__(fr.RigidityState)
    s.num_points, s.K, s.idx = P, K, torch.zeros((P, K), dtype=torch.int32)
    return s


def test_python_refusals_without_a_device():
    import fused_rigidity as fr
    P, K = 10, 4
    xyz, rot = torch.zeros((P, 3)), torch.ones((P, 4))
    idx = torch.zeros((P, K), dtype=torch.int32)
    off, dist, w, pinv = torch.zeros((P, K, 3)), torch.zeros((P, K)), torch.zeros((P, K)), torch.ones((P, 4))
    state = _stub_state(P)
    calls = (fr.rigidity_loss, fr.rigidity_loss_terms, fr.rigidity_loss_and_grads)
    # types
    with pytest.raises(TypeError):
        fr.RigidityState.capture(xyz.numpy(), rot)
    with pytest.raises(TypeError):
        fr.RigidityState.capture(xyz, rot.numpy())
    with pytest.raises(TypeError):
        fr.RigidityState.capture(xyz, rot, K=3.0)
    with pytest.raises(TypeError):
        fr.RigidityState.capture(xyz, rot, K=True)
    with pytest.raises(TypeError):
        fr.RigidityState.capture(xyz, rot, weight_lambda="2000")
    with pytest.raises(TypeError):
        fr.RigidityState.capture(xyz, rot, mask=[True] * P)
    with pytest.raises(TypeError):
        fr.RigidityState.from_tables(idx.numpy(), off, dist, w, pinv, P)
    with pytest.raises(TypeError):
        fr.RigidityState.from_tables(idx, off, dist.numpy(), w, pinv, P)
    with pytest.raises(TypeError):
        fr.RigidityState.from_tables(idx, off, dist, w, pinv, float(P))
    for f in calls:
        with pytest.raises(TypeError):
            f(xyz.numpy(), rot, state)
        with pytest.raises(TypeError):
            f(xyz, rot, (idx, off, dist, w, pinv))
        with pytest.raises(TypeError):
            f(xyz, rot, state, rigid="4")
        with pytest.raises(TypeError):
            f(xyz, rot, state, iso=None)
    # values
    for bad in (0, -1, 33):
        with pytest.raises(ValueError, match="1..32"):
            fr.RigidityState.capture(xyz, rot, K=bad)
    with pytest.raises(ValueError, match="1..32"):
        fr.RigidityState.from_tables(torch.zeros((P, 33), dtype=torch.int32), torch.zeros((P, 33, 3)), torch.zeros((P, 33)), torch.zeros((P, 33)), pinv, P)
    bad = idx.clone()
    bad[3, 1] = P
    with pytest.raises(ValueError, match=r"\[-1, 10\)"):
        fr.RigidityState.from_tables(bad, off, dist, w, pinv, P, check=True)
    with pytest.raises(ValueError, match="unknown gradient"):
        fr.rigidity_loss_and_grads(xyz, rot, state, want=("xyz", "scaling"))
    # shapes and dtypes
    with pytest.raises(RuntimeError, match=r"\(rows, 3\)"):
        fr.RigidityState.capture(torch.zeros((P, 4)), rot)
    with pytest.raises(RuntimeError, match=r"\(rows, 4\)"):
        fr.RigidityState.capture(xyz, torch.zeros((P, 3)))
    with pytest.raises(RuntimeError, match="float32"):
        fr.RigidityState.capture(xyz.double(), rot)
    with pytest.raises(RuntimeError, match="float32"):
        fr.RigidityState.capture(xyz, rot.half())
    with pytest.raises(RuntimeError, match="rotation has 9"):
        fr.RigidityState.capture(xyz, rot[:9])
    with pytest.raises(RuntimeError, match="bool"):
        fr.RigidityState.capture(xyz, rot, mask=torch.ones(P))
    with pytest.raises(RuntimeError, match="mask"):
        fr.RigidityState.capture(xyz, rot, mask=torch.ones(P + 1, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="int32"):
        fr.RigidityState.from_tables(idx.long(), off, dist, w, pinv, P)
    with pytest.raises(RuntimeError, match="one row per point"):
        fr.RigidityState.from_tables(idx, off, dist, w, pinv, P + 1)
    with pytest.raises(RuntimeError, match="prev_offset"):
        fr.RigidityState.from_tables(idx, off[:, :, :2], dist, w, pinv, P)
    with pytest.raises(RuntimeError, match="prev_dist"):
        fr.RigidityState.from_tables(idx, off, dist[:, :3], w, pinv, P)
    with pytest.raises(RuntimeError, match="weight"):
        fr.RigidityState.from_tables(idx, off, dist, w.double(), pinv, P)
    with pytest.raises(RuntimeError, match="prev_inv_rot"):
        fr.RigidityState.from_tables(idx, off, dist, w, pinv[:, :3], P)
    for f in calls:
        with pytest.raises(RuntimeError, match=r"\(rows, 3\)"):
            f(xyz[:, :2], rot, state)
        with pytest.raises(RuntimeError, match="float32"):
            f(xyz, rot.double(), state)
        with pytest.raises(RuntimeError, match="built for 7 points"):
            f(xyz, rot, _stub_state(7))
    # no CPU path
    with pytest.raises(RuntimeError, match="no CPU path"):
        fr.RigidityState.capture(xyz, rot)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fr.RigidityState.capture(xyz, rot, mask=torch.ones(P, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fr.RigidityState.from_tables(idx, off, dist, w, pinv, P)
    for f in calls:
        with pytest.raises(RuntimeError, match="no CPU path"):
            f(xyz, rot, state)
