"""CPU: the extended fused loss (include/gsr_loss_ext.h, fused_loss.training_loss*).  The torch reference of tests/torch_loss_ext.py
with no option reproduces the golden vectors of the reference's own loss_utils.py and the float64 oracle (the bars of test_loss.py);
the header compiles as C99 and as C++17 alongside gsr.h and when included twice; every function it declares is exported; the
scratch size is 0 for sizes that are not positive, monotone and at least the three maps; the entry point validates its arguments
before any device work; the Python surfaces refuse before the kernel library is loaded.  Nothing here touches a device."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import torch_loss_ext as ref
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsr_loss_ext.h")
LIB = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "libgsr_hip.so")
GOLD = os.path.join(ROOT, "tests", "golden", "loss_golden.npz")
INVALID = -1   # GSR_ERR_INVALID_ARGUMENT


def _nerr(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / max(np.abs(b).max(), 1e-30))


def _lib():
    if not os.path.exists(LIB):
        __graft_entry__.build()
    import fused_loss
    L = ctypes.CDLL(LIB)
    L.gsr_last_error.restype = ctypes.c_char_p
    L.gsr_loss_ext_scratch_bytes.restype = ctypes.c_size_t
    L.gsr_loss_ext_scratch_bytes.argtypes = [ctypes.c_int] * 3
    L.gsr_l1_ssim_loss_ext.restype = ctypes.c_int
    L.gsr_l1_ssim_loss_ext.argtypes = [ctypes.POINTER(fused_loss.LossExtArgs)]
    return L


@pytest.mark.parametrize("name", ("noise", "smooth", "equal"))
def test_reference_without_options_is_the_existing_loss(name):
    g = np.load(GOLD)
    img, gt = torch.from_numpy(g[f"{name}_img"]), torch.from_numpy(g[f"{name}_gt"])
    vals, grads = ref.loss_and_grads(img, gt, 0.2)
    vals, grad = vals.numpy(), grads["image"].numpy()
    assert vals[3] == 0.0
    gold = g[f"{name}_vals"]
    assert abs(vals[0] - gold[0]) < 1e-5 and abs(vals[1] - gold[1]) < 1e-6 and abs(vals[2] - gold[2]) < 1e-5, (vals, gold)
    o_loss, o_l1, o_ss, o_grad = oracle.l1_ssim(g[f"{name}_img"], g[f"{name}_gt"], 0.2)
    assert abs(vals[0] - o_loss) < 1e-5 and abs(vals[1] - o_l1) < 1e-6 and abs(vals[2] - o_ss) < 1e-5, (vals, o_loss, o_l1, o_ss)
    if name == "equal":   # SSIM is at its maximum and L1 at its kink: the exact gradient is 0
        assert np.abs(grad).max() < 1e-12
    else:
        assert _nerr(grad, g[f"{name}_grad"]) < 5e-4
        assert _nerr(grad, o_grad) <= 1e-5, _nerr(grad, o_grad)   # the oracle hands its gradient out in float32


def test_struct_layout_matches_the_header():
    import fused_loss
    a = fused_loss.LossExtArgs
    assert ctypes.sizeof(a) == 128 and a.img.offset == 16 and a.invdepth_weight.offset == 72 and a.vals.offset == 80
    assert a.scratch.offset == 112 and a.stream.offset == 120


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_alongside_the_core_abi(tmp_path, compiler, std, ext):
    src = tmp_path / f"includer.{ext}"
    src.write_text('#include "gsr.h"\n#include "gsr_loss_ext.h"\n#include "gsr_loss_ext.h"\n'
                   "int gsr_loss_ext_includer(void) { return (int)(sizeof(&gsr_l1_ssim_loss_ext) + sizeof(&gsr_loss_ext_scratch_bytes) + "
                   "sizeof(gsr_loss_ext_args) + sizeof(&gsr_l1_ssim_loss)); }\n")
    r = subprocess.run([compiler, std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_every_declared_symbol_is_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr)))
    assert names == ["gsr_l1_ssim_loss_ext", "gsr_loss_ext_scratch_bytes"], names
    L = _lib()
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/gsr_loss_ext.h but not exported"


def test_scratch_size_is_zero_for_sizes_that_are_not_positive_and_monotone():
    L = _lib()
    for c, h, w in ((0, 8, 8), (3, 0, 8), (3, 8, 0), (-1, 8, 8), (3, -8, 8), (3, 8, -8), (-3, -3, -3)):
        assert L.gsr_loss_ext_scratch_bytes(c, h, w) == 0, (c, h, w)
    sizes = (1, 2, 7, 31, 32, 33, 63, 64, 65, 130, 1080, 1980, 4096)
    for c in (1, 3, 4):
        for h in sizes:
            prev = 0
            for w in sizes:   # monotone in the width, and room for the three maps
                b = L.gsr_loss_ext_scratch_bytes(c, h, w)
                assert b >= prev and b >= 12 * c * h * w, (c, h, w, b, prev)
                prev = b
        for w in sizes:
            prev = 0
            for h in sizes:   # monotone in the height
                b = L.gsr_loss_ext_scratch_bytes(c, h, w)
                assert b >= prev, (c, h, w, b, prev)
                prev = b
    for h in sizes:
        for w in sizes:   # monotone in the channels
            assert L.gsr_loss_ext_scratch_bytes(1, h, w) <= L.gsr_loss_ext_scratch_bytes(3, h, w) <= L.gsr_loss_ext_scratch_bytes(4, h, w)


def test_entry_point_validates_before_any_device_work():
    import fused_loss
    L = _lib()
    one = 4096   # a non-NULL address that must never be dereferenced
    ok = dict(C=3, H=16, W=32, lambda_dssim=0.2, img=one, gt=one, mask=one, exposure=one, invdepth=one, invdepth_prior=one,
              invdepth_mask=one, invdepth_weight=0.5, vals=one, dL_dimg=one, dL_dexposure=one, dL_dinvdepth=one, scratch=one, stream=None)
    no_depth = dict(invdepth=None, invdepth_prior=None, invdepth_mask=None, dL_dinvdepth=None)
    bad = [dict(C=0), dict(H=0), dict(W=0), dict(C=-3), dict(H=-1), dict(W=-7),
           dict(img=None), dict(gt=None), dict(vals=None), dict(scratch=None),
           dict(C=1), dict(C=4),                                          # exposure needs three channels
           dict(exposure=None),                                           # dL_dexposure without exposure
           dict(invdepth=None), dict(invdepth_prior=None),                # exactly one of the two
           dict(no_depth, invdepth_mask=one), dict(no_depth, dL_dinvdepth=one),
           dict(invdepth_weight=-0.5), dict(invdepth_weight=math.inf), dict(invdepth_weight=math.nan), dict(invdepth_weight=-math.inf)]
    for kw in bad:
        a = fused_loss.LossExtArgs(**dict(ok, **kw))
        assert L.gsr_l1_ssim_loss_ext(ctypes.byref(a)) == INVALID, kw
        assert L.gsr_last_error().startswith(b"gsr_l1_ssim_loss_ext:"), (kw, L.gsr_last_error())
    assert L.gsr_l1_ssim_loss_ext(None) == INVALID
    assert L.gsr_last_error().startswith(b"gsr_l1_ssim_loss_ext:"), L.gsr_last_error()


def test_python_surfaces_refuse_before_the_library_loads():
    import fused_loss
    from diff_gaussian_rasterization import _C
    loaded = _C._lib
    _C._lib = None
    try:
        x, y = torch.rand(3, 8, 12), torch.rand(3, 8, 12)
        p, E = torch.rand(8, 12), torch.eye(3, 4)
        for fn in (fused_loss.training_loss_and_grads, fused_loss.training_loss_terms, fused_loss.training_loss):
            with pytest.raises(RuntimeError, match="HIP"):   # a valid call on CPU tensors: no CPU path
                fn(x, y, 0.2, mask=p, exposure=E, invdepth=p, invdepth_prior=p, invdepth_mask=p, invdepth_weight=0.1)
            with pytest.raises(RuntimeError, match=r"\(C,H,W\)"):
                fn(x, y[:, :7])
            with pytest.raises(RuntimeError, match=r"\(C,H,W\)"):
                fn(x[0], y[0])
            with pytest.raises(RuntimeError, match="float32"):
                fn(x.double(), y.double())
            with pytest.raises(RuntimeError, match="mask"):
                fn(x, y, mask=torch.rand(3, 8, 12))
            with pytest.raises(RuntimeError, match="mask"):
                fn(x, y, mask=p.double())
            with pytest.raises(ValueError, match="exposure"):
                fn(x[:1], y[:1], exposure=E)
            with pytest.raises(RuntimeError, match="exposure"):
                fn(x, y, exposure=torch.eye(4, 4))
            with pytest.raises(ValueError, match="invdepth_prior"):
                fn(x, y, invdepth=p)
            with pytest.raises(ValueError, match="invdepth_prior"):
                fn(x, y, invdepth_prior=p)
            with pytest.raises(ValueError, match="invdepth_mask"):
                fn(x, y, invdepth_mask=p)
            with pytest.raises(RuntimeError, match="invdepth_prior"):
                fn(x, y, invdepth=p, invdepth_prior=torch.rand(12, 8))
            for w in (-1.0, float("inf"), float("nan")):
                with pytest.raises(ValueError, match="invdepth_weight"):
                    fn(x, y, invdepth=p, invdepth_prior=p, invdepth_weight=w)
            with pytest.raises(ValueError, match="want"):
                fn(x, y, want=("image", "gt"))
        assert _C._lib is None, "a refusal loaded the kernel library"
    finally:
        _C._lib = loaded
