"""CPU: the normal-consistency pieces (include/gsr_normals.h, fused_geometry.py, render(normals=)) as far as they go without a device.
The float64 restatement the GPU tests compare against (tests/torch_normals.py) is pinned first: its per-Gaussian normal is the
eigenvector of the covariance for the smallest scale, its depth normals reproduce an analytic plane's normal, its normals face the
camera, and its autograd passes gradcheck.  Then the C ABI: the header compiles as C99 and C++17, every declared function is exported,
the entry points validate before any device work; and the Python surfaces refuse CPU tensors, wrong dtypes and shapes and a non-bool
`normals` before the kernel library is loaded.  Nothing here touches a device."""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import torch_normals as tn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsr_normals.h")
LIB = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "libgsr_hip.so")
INVALID = -1   # GSR_ERR_INVALID_ARGUMENT
NAMES = ["gsr_depth_normals", "gsr_depth_normals_backward", "gsr_gaussian_normals", "gsr_gaussian_normals_backward",
         "gsr_normal_consistency_loss", "gsr_normals_scratch_bytes"]


def _gaussians(P, seed=0):
    import gsr_scene
    g = torch.Generator().manual_seed(seed)
    scales = torch.exp(torch.randn(P, 3, generator=g) * 0.7 - 3.0)
    rot = torch.randn(P, 4, generator=g) * 1.7   # not normalised
    means = torch.rand(P, 3, generator=g) * 3.0 - 1.5
    cam = gsr_scene.ring_camera(200, 120, 1)
    return scales, rot, means, cam.world_view_transform


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def test_restatement_normal_is_the_eigenvector_of_the_smallest_scale():
    import gsr_model
    scales, rot, means, V = _gaussians(200)
    scales[0], scales[1], scales[2] = torch.tensor([.1, .2, .3]), torch.tensor([.2, .1, .3]), torch.tensor([.3, .2, .1])
    scales[3], scales[4], scales[5] = torch.tensor([.1, .1, .3]), torch.tensor([.3, .1, .1]), torch.tensor([.2, .2, .2])   # exact ties
    n, k, sign, _ = tn.gaussian_normals(scales, rot, means, V, "world", parts=True)
    assert k[:6].tolist() == [0, 1, 2, 0, 1, 0] and set(k.tolist()) == {0, 1, 2}
    c = gsr_model.build_covariance_from_scaling_rotation(scales.double(), 1.0, rot.double())
    S = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).view(-1, 3, 3)
    sk2 = scales.double().gather(1, k[:, None])[:, 0] ** 2
    assert torch.allclose(n.norm(dim=1), torch.ones(200, dtype=torch.float64), atol=1e-12)
    err = ((S @ n[:, :, None])[:, :, 0] - sk2[:, None] * n).abs().max() / sk2.max()
    assert float(err) < 1e-12, float(err)
    # the log-scales choose the same axis
    assert torch.equal(tn.min_axis(torch.log(scales)), k)
    # the view-space output is the world-space one rotated by the view matrix's rotation part
    nv = tn.gaussian_normals(scales, rot, means, V, "view")
    assert torch.allclose(nv, n @ V.double()[:3, :3], atol=1e-12)
    # a zero quaternion has no normal
    rot[7] = 0
    q = rot.double().requires_grad_(True)
    nz = tn.gaussian_normals(scales, q, means, V)
    assert nz[7].abs().max() == 0
    nz.sum().backward()
    assert bool(torch.isfinite(q.grad).all()) and q.grad[7].abs().max() == 0 and q.grad[8].abs().max() > 0


def test_restatement_normals_face_the_camera():
    scales, rot, means, V = _gaussians(500, seed=1)
    n, k, sign, cos = tn.gaussian_normals(scales, rot, means, V, "view", parts=True)
    t = means.double() @ V.double()[:3, :3] + V.double()[3, :3]
    assert float((n * t).sum(1).max()) <= 0
    assert (sign > 0).any() and (sign < 0).any()   # both branches of the flip


def test_restatement_depth_normals_of_an_analytic_plane():
    W, H = 70, 37
    tanx = math.tan(0.5)
    tany = tanx * H / W
    z, n = tn.plane_depth(W, H, tanx, tany)
    nd = tn.depth_normals(z.float(), tanx, tany)   # the fp32-rounded depth
    err = float((nd[:, 1:-1, 1:-1] - n[:, None, None]).abs().max())
    print(f"analytic plane {W}x{H}: max err {err:.2e}")
    assert err < 1e-5
    assert float(nd[:, 0].abs().max()) == 0 and float(nd[:, :, -1].abs().max()) == 0   # the border has no normal
    assert float(nd[2, 1:-1, 1:-1].max()) < 0                                            # facing the camera, like the per-Gaussian normals
    front = tn.depth_normals(torch.full((5, 6), 3.0), tanx, tany)[:, 1:-1, 1:-1]
    assert torch.allclose(front, torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64)[:, None, None].expand_as(front), atol=1e-12)
    # an invalid depth takes the normal away from its four axis neighbours only
    zz = z.float().clone()
    zz[10, 20], zz[20, 40] = float("inf"), 0.0
    nd2 = tn.depth_normals(zz, tanx, tany)
    dead = torch.zeros(H, W, dtype=torch.bool)
    for y, x in ((10, 20), (20, 40)):
        for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            dead[yy, xx] = True
    assert float(nd2[:, dead].abs().max()) == 0
    keep = ~dead
    assert torch.equal(nd2[:, keep], nd[:, keep])
    for shape in ((1, 1), (2, 5), (5, 2)):   # no interior pixel
        assert float(tn.depth_normals(torch.ones(shape), tanx, tany).abs().max()) == 0


def test_restatement_gradcheck():
    scales, rot, means, V = _gaussians(6, seed=2)
    q = rot.double().requires_grad_(True)
    for space in ("view", "world"):
        assert torch.autograd.gradcheck(lambda r: tn.gaussian_normals(scales, r, means, V, space), (q,), eps=1e-6, atol=1e-7)
    g = torch.Generator().manual_seed(3)
    H, W = 6, 7
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    z = 3.0 + 0.3 * torch.sin(0.9 * xx) + 0.2 * torch.cos(0.7 * yy) + 0.05 * torch.rand(H, W, generator=g, dtype=torch.float64)
    z[2, 3] = -1.0   # no valid depth, and none within the check's perturbation
    z.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda d: tn.depth_normals(d, 0.5, 0.4), (z,), eps=1e-6, atol=1e-7)
    N = torch.randn(3, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    a = torch.rand(H, W, generator=g, dtype=torch.float64)
    for alpha in (a, None):
        assert torch.autograd.gradcheck(lambda n, d: tn.normal_consistency_loss(n, d, alpha, 0.5, 0.4), (N, z), eps=1e-6, atol=1e-7)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def _lib():
    if not os.path.exists(LIB):
        __graft_entry__.build()
    L = ctypes.CDLL(LIB)
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.gsr_last_error.restype = ctypes.c_char_p
    L.gsr_gaussian_normals.restype = i
    L.gsr_gaussian_normals.argtypes = [i] + [vp] * 4 + [i, vp, vp]
    L.gsr_gaussian_normals_backward.restype = i
    L.gsr_gaussian_normals_backward.argtypes = [i] + [vp] * 4 + [i, vp, vp, vp]
    L.gsr_normals_scratch_bytes.restype = ctypes.c_size_t
    L.gsr_normals_scratch_bytes.argtypes = [i, i]
    L.gsr_depth_normals.restype = i
    L.gsr_depth_normals.argtypes = [i, i, vp, f, f, vp, vp]
    L.gsr_depth_normals_backward.restype = i
    L.gsr_depth_normals_backward.argtypes = [i, i, vp, f, f, vp, vp, vp]
    L.gsr_normal_consistency_loss.restype = i
    L.gsr_normal_consistency_loss.argtypes = [i, i, vp, vp, vp, f, f, vp, vp, vp, vp, vp]
    return L


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_alongside_the_core_abi(tmp_path, compiler, std, ext):
    src = tmp_path / f"includer.{ext}"
    src.write_text('#include "gsr.h"\n#include "gsr_normals.h"\n#include "gsr_normals.h"\n'
                   "int gsr_normals_includer(void) { return (int)(" + " + ".join(f"sizeof(&{n})" for n in NAMES) +
                   ") + GSR_NORMALS_VIEW + GSR_NORMALS_WORLD; }\n")
    r = subprocess.run([compiler, std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_every_declared_symbol_is_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr)))
    assert names == NAMES, names
    L = _lib()
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/gsr_normals.h but not exported"


def test_gaussian_entry_points_validate_before_any_device_work():
    L = _lib()
    one, odd = 4096, 4104   # non-NULL addresses that must never be dereferenced; the second is 8-byte aligned only

    def fwd(P=4, s=one, q=one, m=one, v=one, space=0, out=one):
        return L.gsr_gaussian_normals(P, s, q, m, v, space, out, None)

    def bwd(P=4, s=one, q=one, m=one, v=one, space=1, g=one, dq=one):
        return L.gsr_gaussian_normals_backward(P, s, q, m, v, space, g, dq, None)

    for call, who, bad in ((fwd, b"gsr_gaussian_normals:", [dict(P=-1), dict(s=None), dict(q=None), dict(m=None), dict(v=None), dict(out=None),
                                                            dict(space=2), dict(space=-1), dict(q=odd), dict(P=0, space=7)]),
                           (bwd, b"gsr_gaussian_normals_backward:", [dict(P=-1), dict(s=None), dict(q=None), dict(m=None), dict(v=None),
                                                                     dict(g=None), dict(dq=None), dict(space=2), dict(q=odd), dict(dq=odd)])):
        for kw in bad:
            assert call(**kw) == INVALID, kw
            assert L.gsr_last_error().startswith(who), (kw, L.gsr_last_error())
    # nothing to do: GSR_OK with no launch (an empty array has no address)
    assert fwd(P=0, s=None, q=None, m=None, v=None, out=None) == 0 and L.gsr_last_error() == b""
    assert bwd(P=0, s=None, q=None, m=None, v=None, g=None, dq=None) == 0 and L.gsr_last_error() == b""


def test_image_entry_points_validate_before_any_device_work():
    L = _lib()
    one = 4096
    for w, h in ((-1, 10), (10, -1), (0, 10), (10, 0)):
        assert L.gsr_normals_scratch_bytes(w, h) == 0
    prev = 0
    for w in (1, 63, 64, 65, 200, 1980, 16384):   # room for one float per tile of at most 64 x 16 pixels, monotone
        b = L.gsr_normals_scratch_bytes(w, 1080)
        assert b >= 4 * math.ceil(w / 64) * math.ceil(1080 / 16) and b >= prev and b % 16 == 0, (w, b)
        prev = b

    def fwd(W=32, H=16, d=one, out=one):
        return L.gsr_depth_normals(W, H, d, 0.5, 0.5, out, None)

    def bwd(W=32, H=16, d=one, g=one, dd=one):
        return L.gsr_depth_normals_backward(W, H, d, 0.5, 0.5, g, dd, None)

    def loss(W=32, H=16, n=one, d=one, a=one, vals=one, dn=one, dd=one, scratch=one):
        return L.gsr_normal_consistency_loss(W, H, n, d, a, 0.5, 0.5, vals, dn, dd, scratch, None)

    for call, who, bad in ((fwd, b"gsr_depth_normals:", [dict(W=0), dict(H=-3), dict(d=None), dict(out=None)]),
                           (bwd, b"gsr_depth_normals_backward:", [dict(W=0), dict(H=-3), dict(d=None), dict(g=None), dict(dd=None)]),
                           (loss, b"gsr_normal_consistency_loss:", [dict(W=0), dict(H=-3), dict(n=None), dict(d=None), dict(vals=None),
                                                                    dict(scratch=None), dict(W=-1, a=None, dn=None, dd=None)])):
        for kw in bad:
            assert call(**kw) == INVALID, kw
            assert L.gsr_last_error().startswith(who), (kw, L.gsr_last_error())


# ---- the Python surfaces ---------------------------------------------------------------------------------------------------------------
def test_python_surfaces_refuse_before_anything_runs():
    import fused_geometry as fg
    import gsr_model
    from diff_gaussian_rasterization import _C
    from gaussian_renderer import render
    loaded = _C._lib
    _C._lib = None
    try:
        s, q, m, V = torch.ones(4, 3), torch.ones(4, 4), torch.zeros(4, 3), torch.eye(4)
        with pytest.raises(RuntimeError, match="HIP"):
            fg.gaussian_normals(s, q, m, V)                         # CPU tensors
        with pytest.raises(RuntimeError, match="float32"):
            fg.gaussian_normals(s, q.double(), m, V)
        with pytest.raises(RuntimeError, match="float32"):
            fg.gaussian_normals(s.half(), q, m, V)
        with pytest.raises(RuntimeError, match="shape"):
            fg.gaussian_normals(s, torch.ones(4, 3), m, V)
        with pytest.raises(RuntimeError, match="shape"):
            fg.gaussian_normals(torch.ones(5, 3), q, m, V)
        with pytest.raises(TypeError, match="tensor"):
            fg.gaussian_normals(s, None, m, V)
        for bad in ("camera", 0, None):
            with pytest.raises(ValueError, match="space"):
                fg.gaussian_normals(s, q, m, V, space=bad)
        d, n, a = torch.ones(8, 9), torch.ones(3, 8, 9), torch.ones(1, 8, 9)
        with pytest.raises(RuntimeError, match="HIP"):
            fg.depth_normals(d, 0.5, 0.5)
        with pytest.raises(RuntimeError, match="HIP"):
            fg.depth_normals(d[None], 0.5, 0.5)
        with pytest.raises(RuntimeError, match="float32"):
            fg.depth_normals(d.double(), 0.5, 0.5)
        for bad in (torch.ones(2, 8, 9), torch.ones(8), torch.ones(1, 1, 8, 9), torch.ones(0, 9)):
            with pytest.raises(RuntimeError, match="shape"):
                fg.depth_normals(bad, 0.5, 0.5)
        with pytest.raises(TypeError, match="number"):
            fg.depth_normals(d, "wide", 0.5)
        with pytest.raises(TypeError, match="tensor"):
            fg.depth_normals([[1.0]], 0.5, 0.5)
        with pytest.raises(RuntimeError, match="HIP"):
            fg.normal_consistency_loss(n, d, a, 0.5, 0.5)
        with pytest.raises(RuntimeError, match="float32"):
            fg.normal_consistency_loss(n, d.double(), None, 0.5, 0.5)
        with pytest.raises(RuntimeError, match="shape"):
            fg.normal_consistency_loss(n, torch.ones(3, 8, 9), None, 0.5, 0.5)
        # render(normals=): a switch, nothing else
        cam = None
        pc = gsr_model.GaussianParams.from_activated(torch.zeros(4, 3), torch.zeros(4, 1, 3), torch.ones(4, 3), q, torch.ones(4, 1) * 0.5,
                                                     max_sh_degree=0, active_sh_degree=0)
        for bad in (1, 0, "yes", None, torch.ones(1)):
            with pytest.raises(TypeError, match="normals must be a bool"):
                render(cam, pc, gsr_model.pipeline_params(), torch.zeros(3), normals=bad)
        for bad in (1, "view"):
            with pytest.raises(TypeError, match="bool"):
                _C.normals_flag(bad)
        assert _C.normals_flag(True) is True and _C.normals_flag(False) is False
        assert _C._lib is None, "a refusal loaded the kernel library"
    finally:
        _C._lib = loaded
