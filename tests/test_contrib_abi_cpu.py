"""CPU: the C ABI of the blend-weight statistics (include/gsr_contrib.h) compiles as C99 and as C++17, every function it declares is
exported by the built library, gsr_contributions validates its arguments before any device work, and the Python surfaces refuse CPU
tensors, wrong dtypes and wrong shapes before a kernel is loaded.  Nothing here touches a device."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsr_contrib.h")
LIB = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "libgsr_hip.so")


def _lib():
    if not os.path.exists(LIB):
        __graft_entry__.build()
    L = ctypes.CDLL(LIB)
    L.gsr_last_error.restype = ctypes.c_char_p
    L.gsr_contrib_scratch_bytes.restype = ctypes.c_size_t
    L.gsr_contrib_scratch_bytes.argtypes = [ctypes.c_int, ctypes.c_int64]
    L.gsr_contributions.restype = ctypes.c_int
    L.gsr_contributions.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 9 + [ctypes.c_int]
    return L


def _declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr)))


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles(tmp_path, compiler, std, ext):
    src = tmp_path / f"includer.{ext}"
    src.write_text('#include "gsr_contrib.h"\nint gsr_contrib_includer(void) { return (int)sizeof(&gsr_contributions); }\n')
    r = subprocess.run([compiler, std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_every_declared_symbol_is_exported():
    names = _declared()
    assert names == ["gsr_contrib_scratch_bytes", "gsr_contributions"], names
    L = _lib()
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/gsr_contrib.h but not exported"


def test_scratch_size_is_monotone():
    L = _lib()
    assert L.gsr_contrib_scratch_bytes(10, -1) == 0
    prev = L.gsr_contrib_scratch_bytes(10, 0)
    for R in (1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 100_000, 100_001, 10_000_000, 1 << 31, (1 << 32) - 1):
        b = L.gsr_contrib_scratch_bytes(10, R)
        assert b >= prev and b >= 17 * R, (R, b, prev)   # a 16-byte record and a validity byte per slot
        assert b % 16 == 0
        prev = b
    assert L.gsr_contrib_scratch_bytes(10, 5000) == L.gsr_contrib_scratch_bytes(10_000_000, 5000)


def test_validation_before_any_device_work():
    L = _lib()
    one = ctypes.c_void_p(4096)   # a non-NULL, 16-byte aligned address that must never be dereferenced

    def call(P=4, R=8, W=32, H=16, geom=one, binning=one, image=one, pw=None, ws=one, wm=one, pc=one, scratch=one):
        return L.gsr_contributions(P, R, W, H, geom, binning, image, pw, ws, wm, pc, scratch, None, 0)

    bad = [dict(P=-1), dict(R=-1), dict(W=0), dict(H=-3), dict(geom=None), dict(image=None), dict(binning=None),
           dict(ws=None, wm=None, pc=None), dict(scratch=None)]
    for kw in bad:
        assert call(**kw) == -1, kw   # GSR_ERR_INVALID_ARGUMENT
        assert L.gsr_last_error(), kw
    assert b"outputs" in (call(ws=None, wm=None, pc=None), L.gsr_last_error())[1]
    # nothing to do: GSR_OK with no launch (no state, no scratch needed)
    assert call(P=0, geom=None, binning=None, image=None, scratch=None) == 0
    assert call(P=0, geom=None, binning=None, image=None, scratch=None, ws=None, wm=None, pc=None) == 0   # empty arrays have no address
    assert call(R=0, binning=None, scratch=None) == 0
    assert call(R=0, binning=None, scratch=None, ws=None, wm=None) == 0   # one output is enough
    assert L.gsr_last_error() == b""


def test_python_surfaces_refuse_cpu_tensors_and_wrong_dtypes():
    import diff_gaussian_rasterization as dgr
    import fused_params
    import gaussian_renderer  # noqa: F401  (imports with the new keywords)
    from diff_gaussian_rasterization import _C
    loaded = _C._lib
    _C._lib = None
    try:
        e = torch.empty(0, dtype=torch.uint8)
        f, i = torch.zeros(4), torch.zeros(4, dtype=torch.int32)
        with pytest.raises(RuntimeError, match="no CPU path"):
            _C.gaussian_contributions(e, e, e, 8, 4, 32, 16, (f, f.clone(), i))
        with pytest.raises(RuntimeError, match="no CPU path"):
            _C.gaussian_contributions(e, e, e, 8, 4, 32, 16, (None, None, i))
        with pytest.raises(RuntimeError, match="weight_sum must be float32"):
            _C.gaussian_contributions(e, e, e, 8, 4, 32, 16, (f.double(), None, None))
        with pytest.raises(RuntimeError, match="pixel_count must be int32"):
            _C.gaussian_contributions(e, e, e, 8, 4, 32, 16, (None, None, f))
        with pytest.raises(RuntimeError, match="P = 4 elements"):
            _C.gaussian_contributions(e, e, e, 8, 4, 32, 16, (None, torch.zeros(5), None))
        with pytest.raises(RuntimeError, match="P = 4 elements"):
            _C.gaussian_contributions(e, e, e, 8, 4, 32, 16, (torch.zeros(4, 1), None, None))
        with pytest.raises(RuntimeError, match="at least one"):
            _C.gaussian_contributions(e, e, e, 8, 4, 32, 16, (None, None, None))
        for bad_map, msg in ((torch.zeros(32, 16), "shape"), (torch.zeros(16, 32, dtype=torch.float64), "float32")):
            with pytest.raises(RuntimeError, match=msg):
                _C.contrib_pixel_weight(bad_map, 32, 16, torch.device("cpu"))
        # the module and the leaf path check the statistics before the forward runs
        s = dgr.GaussianRasterizationSettings(16, 16, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                              torch.zeros(3), False, False)
        m = torch.zeros(4, 3)
        with pytest.raises(RuntimeError, match="weight_max must be a HIP"):
            dgr.GaussianRasterizer(s, contrib_stats=(None, f, None))(means3D=m, means2D=m, opacities=torch.zeros(4, 1), shs=torch.zeros(4, 1, 3),
                                                                     scales=m, rotations=torch.zeros(4, 4))
        with pytest.raises(RuntimeError, match="pixel_count must be int32"):
            fused_params.rasterize_leaf_gaussians(m, m, torch.zeros(4, 1, 3), torch.zeros(4, 0, 3), torch.zeros(4, 1), m, torch.zeros(4, 4), s,
                                                  contrib_stats=(None, None, torch.zeros(4, dtype=torch.int64)))
        assert _C._lib is None, "a refusal loaded the kernel library"
    finally:
        _C._lib = loaded
