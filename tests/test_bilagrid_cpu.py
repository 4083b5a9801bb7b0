"""CPU: the bilateral grid of affine colour transforms (include/gsr_bilagrid.h, fused_bilagrid.py).  The hand-written reference of
tests/torch_bilagrid.py equals the stock sequence it restates -- F.grid_sample(bilinear, align_corners=True, padding_mode="border")
at pixel centres followed by the affine product -- in float64, values and both gradients, pixels with out-of-range luma included;
its total variation equals the index-select formulation and that one's autograd gradient.  The header compiles as C99 and as C++17
beside gsr.h and when included twice; every function it declares is exported; both scratch functions return 0 for invalid sizes and
are monotone in each argument; every entry point validates its arguments before any device work; the Python surfaces refuse before
the kernel library is loaded.  Nothing here touches a device."""
import ctypes
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import torch_bilagrid as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsr_bilagrid.h")
LIB = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "libgsr_hip.so")
INVALID = -1   # GSR_ERR_INVALID_ARGUMENT
SLICE_SHAPES = (((7, 9), (2, 2, 2)), ((33, 65), (8, 16, 16)), ((70, 130), (3, 2, 5)))
TV_SHAPES = ((1, 12, 2, 2, 2), (3, 12, 8, 16, 16), (2, 12, 3, 2, 5), (12, 4, 3, 6))


def _lib():
    if not os.path.exists(LIB):
        __graft_entry__.build()
    import fused_bilagrid
    L = ctypes.CDLL(LIB)
    L.gsr_last_error.restype = ctypes.c_char_p
    L.gsr_bilagrid_scratch_bytes.restype = ctypes.c_size_t
    L.gsr_bilagrid_scratch_bytes.argtypes = [ctypes.c_int] * 5
    L.gsr_bilagrid_tv_scratch_bytes.restype = ctypes.c_size_t
    L.gsr_bilagrid_tv_scratch_bytes.argtypes = [ctypes.c_int] * 4
    for name in ("gsr_bilagrid_slice", "gsr_bilagrid_slice_backward"):
        getattr(L, name).restype = ctypes.c_int
        getattr(L, name).argtypes = [ctypes.POINTER(fused_bilagrid.BilagridArgs)]
    L.gsr_bilagrid_tv.restype = ctypes.c_int
    L.gsr_bilagrid_tv.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 5
    return L


def _stock_slice(grid, image):
    """the sequence a user writes in stock PyTorch (gsplat's slice, pixel-centre coordinates)"""
    _, L, GH, GW = grid.shape
    _, H, W = image.shape
    ys, xs = torch.meshgrid((torch.arange(H, dtype=grid.dtype) + 0.5) / H, (torch.arange(W, dtype=grid.dtype) + 0.5) / W, indexing="ij")
    luma = torch.tensor(ref.LUMA, dtype=grid.dtype) @ image.reshape(3, -1)
    coords = torch.stack([xs, ys, luma.reshape(H, W)], dim=-1) * 2 - 1                      # (H, W, 3) in [-1, 1]: x, y, z
    A = F.grid_sample(grid[None], coords[None, None], mode="bilinear", align_corners=True, padding_mode="border")   # (1, 12, 1, H, W)
    A = A[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
    rgb1 = torch.cat([image, torch.ones_like(image[:1])]).permute(1, 2, 0)                  # (H, W, 4)
    return torch.matmul(A, rgb1[..., None])[..., 0].permute(2, 0, 1)


@pytest.mark.parametrize("hw,lgg", SLICE_SHAPES)
def test_reference_equals_the_grid_sample_sequence_in_float64(hw, lgg):
    grid, image, grad_out = ref.make_inputs(*hw, *lgg)
    ref.assert_inputs_are_safe(image, *lgg)
    out, grads, _, inside = ref.slice_and_grads(grid, image, grad_out)
    assert bool((~inside).any())
    g = grid.double().requires_grad_(True)
    x = image.double().requires_grad_(True)
    stock = _stock_slice(g, x)
    dg, dx = torch.autograd.grad(stock, (g, x), grad_out.double())
    errs = (float((out - stock.detach()).abs().max()), float((grads["grid"] - dg).abs().max()), float((grads["image"] - dx).abs().max()))
    print(f"{hw} / {lgg}: out {errs[0]:.1e}, d/dgrid {errs[1]:.1e}, d/dimage {errs[2]:.1e}")
    assert errs[0] <= 1e-12 and errs[1] <= 1e-11 and errs[2] <= 1e-11, errs
    # at a clamped pixel the guidance part is zero: the affine part alone, in the reference and in the stock sequence
    _, _, affine, _ = ref.slice_and_grads(grid, image, grad_out)
    assert float((grads["image"] - affine)[:, ~inside].abs().max()) <= 1e-13 and float((dx - affine)[:, ~inside].abs().max()) <= 1e-11
    assert float((grads["image"] - affine)[:, inside].abs().max()) > 1e-3


@pytest.mark.parametrize("shape", TV_SHAPES)
def test_tv_reference_equals_the_index_select_formulation(shape):
    g = torch.randn(*shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    tv, dg = ref.tv_and_grad(g)
    x = g.clone().requires_grad_(True)
    x5 = x if x.dim() == 5 else x[None]
    N = x5.shape[0]
    total = 0
    for axis in (2, 3, 4):   # gsplat's total_variation_loss: index_select of the two shifted halves
        n = x5.shape[axis]
        a = x5.index_select(axis, torch.arange(1, n)) - x5.index_select(axis, torch.arange(0, n - 1))
        total = total + a.square().sum() / (12 * a.shape[2] * a.shape[3] * a.shape[4])
    total = total / N
    (dx,) = torch.autograd.grad(total, x)
    assert abs(float(tv) - float(total.detach())) <= 1e-12 * abs(float(total.detach()))
    assert float((dg - dx).abs().max()) <= 1e-12 * float(dx.abs().max())


def test_struct_layout_matches_the_header():
    import fused_bilagrid
    a = fused_bilagrid.BilagridArgs
    assert ctypes.sizeof(a) == 88 and a.GW.offset == 16 and a.grid.offset == 24 and a.out.offset == 40 and a.dL_dout.offset == 48
    assert a.dL_dgrid.offset == 56 and a.dL_dimg.offset == 64 and a.scratch.offset == 72 and a.stream.offset == 80


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_alongside_the_core_abi(tmp_path, compiler, std, ext):
    src = tmp_path / f"includer.{ext}"
    src.write_text('#include "gsr.h"\n#include "gsr_bilagrid.h"\n#include "gsr_bilagrid.h"\n'
                   "int gsr_bilagrid_includer(void) { return (int)(sizeof(&gsr_bilagrid_slice) + sizeof(&gsr_bilagrid_slice_backward) + "
                   "sizeof(&gsr_bilagrid_scratch_bytes) + sizeof(&gsr_bilagrid_tv) + sizeof(&gsr_bilagrid_tv_scratch_bytes) + "
                   "sizeof(gsr_bilagrid_args) + sizeof(&gsr_l1_ssim_loss)); }\n")
    r = subprocess.run([compiler, std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_every_declared_symbol_is_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr)))
    assert names == ["gsr_bilagrid_scratch_bytes", "gsr_bilagrid_slice", "gsr_bilagrid_slice_backward", "gsr_bilagrid_tv",
                     "gsr_bilagrid_tv_scratch_bytes"], names
    L = _lib()
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/gsr_bilagrid.h but not exported"


def test_scratch_sizes_are_zero_for_invalid_sizes_and_monotone():
    L = _lib()
    ok = dict(H=8, W=8, L=4, GH=4, GW=4)
    for kw in (dict(H=0), dict(W=0), dict(H=-1), dict(W=-5), dict(L=1), dict(GH=1), dict(GW=1), dict(L=0), dict(GH=-2), dict(GW=0),
               dict(H=46341, W=46341), dict(L=1 << 10, GH=1 << 10, GW=1 << 10)):
        assert L.gsr_bilagrid_scratch_bytes(*dict(ok, **kw).values()) == 0, kw
    for n, l, gh, gw in ((0, 4, 4, 4), (-1, 4, 4, 4), (1, 1, 4, 4), (1, 4, 1, 4), (1, 4, 4, 1), (1, 0, 4, 4), (1 << 12, 1 << 8, 1 << 8, 1 << 8)):
        assert L.gsr_bilagrid_tv_scratch_bytes(n, l, gh, gw) == 0, (n, l, gh, gw)
    pixels, nodes = (1, 2, 7, 33, 64, 65, 130, 1080, 1980, 4096), (2, 3, 4, 5, 8, 9, 16, 17, 64)
    assert L.gsr_bilagrid_scratch_bytes(1080, 1980, 8, 16, 16) > 0

    def monotone(fn, base, axis, values):
        prev = 0
        for v in values:
            args = list(base)
            args[axis] = v
            b = fn(*args)
            assert b > 0 and b % 16 == 0 and b >= prev, (fn.__name__, args, b, prev)
            prev = b

    for h in (1, 33, 1080):
        for w in (1, 65, 1980):
            for l in (2, 5, 8):
                for gh in (2, 7, 16):
                    for gw in (2, 9, 16):
                        base = (h, w, l, gh, gw)
                        monotone(L.gsr_bilagrid_scratch_bytes, base, 0, pixels)
                        monotone(L.gsr_bilagrid_scratch_bytes, base, 1, pixels)
                        for axis in (2, 3, 4):
                            monotone(L.gsr_bilagrid_scratch_bytes, base, axis, nodes)
    for n in (1, 3, 200):
        for l in (2, 5, 8):
            for gh in (2, 7, 16):
                for gw in (2, 9, 16):
                    base = (n, l, gh, gw)
                    monotone(L.gsr_bilagrid_tv_scratch_bytes, base, 0, (1, 2, 3, 10, 200, 1000))
                    for axis in (1, 2, 3):
                        monotone(L.gsr_bilagrid_tv_scratch_bytes, base, axis, nodes)


def test_entry_points_validate_before_any_device_work():
    import fused_bilagrid
    L = _lib()
    one = 4096   # a non-NULL address that must never be dereferenced
    ok = dict(H=16, W=32, L=4, GH=3, GW=5, grid=one, img=one, out=one, dL_dout=one, dL_dgrid=one, dL_dimg=one, scratch=one, stream=None)
    sizes = [dict(H=0), dict(W=0), dict(H=-1), dict(W=-7), dict(L=1), dict(GH=1), dict(GW=1), dict(L=0), dict(GH=-3), dict(GW=0),
             dict(H=46341, W=46341),                        # 3 H W exceeds 32-bit indexing
             dict(L=1 << 10, GH=1 << 10, GW=1 << 10),       # 12 L GH GW does
             dict(H=1 << 29, W=1)]                        # more workgroups than one launch takes
    for name, more in (("gsr_bilagrid_slice", [dict(grid=None), dict(img=None), dict(out=None)]),
                       ("gsr_bilagrid_slice_backward", [dict(grid=None), dict(img=None), dict(dL_dout=None), dict(dL_dgrid=None, dL_dimg=None),
                                                        dict(scratch=None)])):
        fn = getattr(L, name)
        for kw in sizes + more:
            a = fused_bilagrid.BilagridArgs(**dict(ok, **kw))
            assert fn(ctypes.byref(a)) == INVALID, (name, kw)
            assert L.gsr_last_error().startswith(name.encode() + b":"), (name, kw, L.gsr_last_error())
        assert fn(None) == INVALID
        assert L.gsr_last_error().startswith(name.encode() + b":"), L.gsr_last_error()

    def tv(N=2, L_=4, GH=3, GW=5, grids=one, val=one, dgrids=one, scratch=one):
        return L.gsr_bilagrid_tv(N, L_, GH, GW, grids, val, dgrids, scratch, None)

    for kw in (dict(N=0), dict(N=-2), dict(L_=1), dict(GH=1), dict(GW=1), dict(L_=0), dict(GW=-1), dict(grids=None), dict(val=None),
               dict(scratch=None), dict(N=1 << 12, L_=1 << 8, GH=1 << 8, GW=1 << 8)):
        assert tv(**kw) == INVALID, kw
        assert L.gsr_last_error().startswith(b"gsr_bilagrid_tv:"), (kw, L.gsr_last_error())


def test_python_surfaces_refuse_before_the_library_loads():
    import fused_bilagrid as fb
    from diff_gaussian_rasterization import _C
    loaded = _C._lib
    _C._lib = None
    try:
        grid, image, go = torch.rand(12, 4, 3, 5), torch.rand(3, 8, 12), torch.rand(3, 8, 12)
        bg = fb.BilateralGrid(2, grid_X=5, grid_Y=3, grid_W=4)
        surfaces = (lambda g, x: fb.bilateral_grid_slice(g, x), lambda g, x: fb.slice_and_grads(g, x, torch.rand(*x.shape).to(x.dtype)))
        for fn in surfaces:
            with pytest.raises(RuntimeError, match="no CPU path"):   # a valid call on CPU tensors
                fn(grid, image)
            with pytest.raises(RuntimeError, match="float32"):
                fn(grid.double(), image.double())
            with pytest.raises(RuntimeError, match="float32"):
                fn(grid, image.half())
            for bad in (torch.rand(8, 12), torch.rand(1, 8, 12), torch.rand(4, 8, 12), torch.rand(1, 3, 8, 12), torch.rand(3, 0, 12)):
                with pytest.raises(RuntimeError, match=r"\(3, H, W\)"):
                    fn(grid, bad)
            for bad in (torch.rand(4, 3, 5), torch.rand(11, 4, 3, 5), torch.rand(1, 12, 4, 3, 5), torch.rand(3, 4, 4, 3, 5)):
                with pytest.raises(RuntimeError, match=r"\(12, L, GH, GW\)"):
                    fn(bad, image)
            for bad in (torch.rand(12, 1, 3, 5), torch.rand(12, 4, 1, 5), torch.rand(12, 4, 3, 1)):
                with pytest.raises(RuntimeError, match="at least 2"):
                    fn(bad, image)
            with pytest.raises(TypeError):
                fn([[1.0]], image)
        with pytest.raises(RuntimeError, match="grad_out"):
            fb.slice_and_grads(grid, image, go[:, :7])
        with pytest.raises(ValueError, match="want"):
            fb.slice_and_grads(grid, image, go, want=("grid", "gt"))
        with pytest.raises(ValueError, match="want"):
            fb.slice_and_grads(grid, image, go, want=())
        with pytest.raises(RuntimeError, match="no CPU path"):
            bg(image, 1)
        for fn in (fb.total_variation_loss, fb.tv_and_grad):
            with pytest.raises(RuntimeError, match="no CPU path"):
                fn(bg.grids)
            with pytest.raises(RuntimeError, match="no CPU path"):
                fn(grid)
            with pytest.raises(RuntimeError, match="float32"):
                fn(grid.double())
            for bad in (torch.rand(4, 3, 5), torch.rand(2, 2, 12, 4, 3, 5), torch.rand(12)):
                with pytest.raises(RuntimeError, match=r"\(N, 12, L, GH, GW\) or \(12, L, GH, GW\)"):
                    fn(bad)
            for bad in (torch.rand(2, 11, 4, 3, 5), torch.rand(13, 4, 3, 5)):
                with pytest.raises(RuntimeError, match=r"\(12, L, GH, GW\)"):
                    fn(bad)
            for bad in (torch.rand(2, 12, 1, 3, 5), torch.rand(12, 4, 3, 1), torch.rand(0, 12, 4, 3, 5)):
                with pytest.raises(RuntimeError, match="at least"):
                    fn(bad)
        with pytest.raises(RuntimeError, match="no CPU path"):
            bg.tv_loss()
        with pytest.raises(ValueError):
            fb.BilateralGrid(0)
        with pytest.raises(ValueError):
            fb.BilateralGrid(2, grid_W=1)
        assert _C._lib is None, "a refusal loaded the kernel library"
    finally:
        _C._lib = loaded


def test_module_parameter_is_the_identity():
    import fused_bilagrid as fb
    bg = fb.BilateralGrid(2)
    assert [n for n, _ in bg.named_parameters()] == ["grids"]
    assert tuple(bg.grids.shape) == (2, 12, 8, 16, 16) and bg.grids.dtype == torch.float32 and bg.grids.is_contiguous() and bg.grids.requires_grad
    eye = torch.eye(3, 4).reshape(1, 12, 1, 1, 1)
    assert torch.equal(bg.grids.detach(), eye.expand(2, 12, 8, 16, 16))
    small = fb.BilateralGrid(3, grid_X=5, grid_Y=2, grid_W=3)
    assert tuple(small.grids.shape) == (3, 12, 3, 2, 5)
    # the identity grid leaves an image as it is, and has no variation
    x = torch.rand(3, 6, 7, dtype=torch.float64)
    assert float((ref.slice(small.grids[1].detach().double(), x) - x).abs().max()) <= 1e-15
    assert float(ref.total_variation(small.grids.detach().double())) == 0.0
