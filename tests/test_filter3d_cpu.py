"""CPU: Mip-Splatting's 3D smoothing filter (include/gsr_filter3d.h, fused_filter3d.py).  The reference of tests/torch_filter3d.py
equals, in float64, the stock sequence a user writes: the per-camera loop with distance[valid] = min(...), prod and sqrt(det1 / det2),
the reset through inverse_sigmoid.  The stock fp32 activation returns a NaN gradient at log-scale -20 with f = 1e-3 where the per-axis
form is finite.  The header compiles as C99 and as C++17 beside gsr.h and when included twice; every function it declares is
exported; the ctypes record is the header's; the scratch function returns 0 for invalid sizes; every entry point validates its
arguments before any device work; the Python surfaces refuse before the kernel library is loaded.  The scenes of the GPU sweep test
have at most 1 % ambiguous rows, and never the row that sets the fill value.  Nothing here touches a device."""
import ctypes
import math
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import torch_filter3d as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsr_filter3d.h")
LIB = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "libgsr_hip.so")
INVALID = -1   # GSR_ERR_INVALID_ARGUMENT
NAMES = ["gsr_filter3d_activate", "gsr_filter3d_activate_backward", "gsr_filter3d_bake", "gsr_filter3d_compute", "gsr_filter3d_reset_opacity",
         "gsr_filter3d_scratch_bytes"]


def _lib():
    if not os.path.exists(LIB):
        __graft_entry__.build()
    vp = ctypes.c_void_p
    L = ctypes.CDLL(LIB)
    L.gsr_last_error.restype = ctypes.c_char_p
    L.gsr_filter3d_scratch_bytes.restype = ctypes.c_size_t
    L.gsr_filter3d_scratch_bytes.argtypes = [ctypes.c_int]
    L.gsr_filter3d_compute.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp, vp, vp]
    L.gsr_filter3d_activate.argtypes = L.gsr_filter3d_bake.argtypes = [ctypes.c_int] + [vp] * 6
    L.gsr_filter3d_activate_backward.argtypes = [ctypes.c_int] + [vp] * 8
    L.gsr_filter3d_reset_opacity.argtypes = [ctypes.c_int, vp, vp, vp, ctypes.c_double, vp, vp, vp]
    return L


@pytest.mark.parametrize("per_camera", (False, True))
@pytest.mark.parametrize("P,C", ((63, 2), (257, 3), (4099, 17)))
def test_sweep_reference_equals_the_stock_loop_in_float64(P, C, per_camera):
    import fused_filter3d as ff
    xyz, cams = ref.sweep_scene(P, C)
    r = ref.sweep(xyz, ff.pack_cameras(cams, "cpu"), per_camera)
    stock = ref.stock_sweep(xyz, cams, per_camera)
    # the stock product takes sqrt(0.2) in double where the reference takes the fp32 constant of the stock fp32 run
    stock = stock * (ref.ROOT02 / 0.2 ** 0.5)
    err = float(((r.filter[:, None] - stock).abs() / stock).max())
    print(f"P = {P}, C = {C}, per_camera = {per_camera}: reference against the stock loop in float64: {err:.1e}; {int((~r.seen).sum())} rows valid nowhere")
    assert err <= 1e-12
    assert bool(r.seen.any()) and not bool(r.seen.all())


def test_packed_records_hold_the_camera():
    import fused_filter3d as ff
    from diff_gaussian_rasterization import CameraModel
    cams = ref.ring_cameras(3)
    cams[1].camera_model = CameraModel("pinhole", 61.0, 62.0, 30.5, 25.25)
    rec = ff.pack_cameras(cams, "cpu")
    assert rec.shape == (3, ff.CAMERA_FLOATS) and rec.dtype == torch.float32
    x = torch.randn(5, 3)
    for c, cam in enumerate(cams):
        want = x @ cam.world_view_transform[:3, :3] + cam.world_view_transform[3, :3]
        got = x @ rec[c, :9].reshape(3, 3).T + rec[c, 9:12]
        assert torch.allclose(got, want, atol=1e-6)
        assert float(rec[c, 16]) == 64.0 and float(rec[c, 17]) == 48.0 and float(rec[c, 18]) == 0.0 and float(rec[c, 19]) == 0.0
    f0 = 50.0
    assert abs(float(rec[0, 12]) - f0) < 1e-4 and abs(float(rec[0, 13]) - f0) < 1e-4 and float(rec[0, 14]) == 32.0 and float(rec[0, 15]) == 24.0
    assert [float(v) for v in rec[1, 12:16]] == [61.0, 62.0, 30.5, 25.25]
    cams[2].camera_model = CameraModel("fisheye", 60.0, 60.0, 32.0, 24.0)
    with pytest.raises(NotImplementedError, match="fisheye"):
        ff.pack_cameras(cams, "cpu")


@pytest.mark.parametrize("P", (1, 257))
def test_activation_and_reset_references_equal_the_stock_sequence_in_float64(P):
    opacity, scaling, f = ref.make_leaves(P, seed=P)
    opac, scales, _ = ref.activations(opacity, scaling, f)
    s_opac, s_scales = ref.stock_activations(opacity, scaling, f, torch.float64)
    assert float(((opac - s_opac).abs() / opac).max()) <= 1e-12 and float(((scales - s_scales).abs() / scales).max()) <= 1e-12
    # the gradients against autograd through the stock sequence
    l, ls = opacity.double().requires_grad_(True), scaling.double().requires_grad_(True)
    g = torch.Generator().manual_seed(P + 1)
    g_o, g_s = torch.randn(P, 1, generator=g, dtype=torch.float64), torch.randn(P, 3, generator=g, dtype=torch.float64)
    o, s = ref.stock_activations(l, ls, f, torch.float64)
    a_l, a_ls = torch.autograd.grad((o * g_o).sum() + (s * g_s).sum(), (l, ls))
    d_l, t1, t2 = ref.activation_grads(opacity, scaling, f, g_o, g_s)
    assert float(((d_l - a_l).abs() / d_l.abs()).max()) <= 1e-12
    assert float(((t1 + t2 - a_ls).abs() / (t1.abs() + t2.abs())).max()) <= 1e-12
    new, changed = ref.reset_logits(opacity, scaling, f, 0.01)
    stock = ref.stock_reset_logits(opacity, scaling, f, 0.01)
    assert float(((new - stock).abs() / new.abs().clamp(min=1.0)).max()) <= 1e-12
    if P > 1:
        assert bool(changed.any()) and not bool(changed.all())
    assert torch.equal(new[~changed], opacity.double()[~changed])


def test_stock_fp32_gradient_is_nan_where_the_per_axis_form_is_finite():
    opacity, f = torch.zeros(1, 1), torch.full((1, 1), 1e-3)
    scaling = torch.full((1, 3), -20.0, requires_grad=True)
    o, s = ref.stock_activations(opacity, scaling, f, torch.float32)
    assert float(o.detach()) == 0.0   # prod(s^2) = exp(-120) underflows
    (o.sum() + s.sum()).backward()
    assert bool(torch.isnan(scaling.grad).any())
    opac, scales, _ = ref.activations(opacity, scaling.detach(), f)
    d_l, t1, t2 = ref.activation_grads(opacity, scaling.detach(), f, torch.ones(1, 1), torch.ones(1, 3))
    for t in (opac, scales, d_l, t1, t2):
        assert bool(torch.isfinite(t).all())
    assert 0.0 < float(opac) < 1e-15 and float(t2.min()) > 0.0


def test_record_layout_and_constants_match_the_header():
    import fused_filter3d as ff
    assert ctypes.sizeof(ff.FilterCamera) == 80 and ff.FilterCamera.t.offset == 36 and ff.FilterCamera.fx.offset == 48
    assert ff.FilterCamera.W.offset == 64 and ff.FilterCamera.pad.offset == 72
    hdr = open(HDR).read()
    defines = dict(re.findall(r"#define (GSR_FILTER3D_[A-Z_]+) ([0-9.]+)", hdr))
    assert int(defines["GSR_FILTER3D_THREADS"]) == ff.THREADS
    assert int(defines["GSR_FILTER3D_CAMERA_FLOATS"]) == ff.CAMERA_FLOATS == ctypes.sizeof(ff.FilterCamera) // 4
    assert float(defines["GSR_FILTER3D_UNSEEN"]) == ff.UNSEEN == ref.UNSEEN


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_alongside_the_core_abi(tmp_path, compiler, std, ext):
    src = tmp_path / f"includer.{ext}"
    src.write_text('#include "gsr.h"\n#include "gsr_filter3d.h"\n#include "gsr_filter3d.h"\n'
                   "int gsr_filter3d_includer(void) { return (int)(sizeof(&gsr_filter3d_compute) + sizeof(&gsr_filter3d_activate) + "
                   "sizeof(&gsr_filter3d_activate_backward) + sizeof(&gsr_filter3d_bake) + sizeof(&gsr_filter3d_reset_opacity) + "
                   "sizeof(&gsr_filter3d_scratch_bytes) + sizeof(gsr_filter3d_camera) + sizeof(&gsr_adam_step)) + GSR_FILTER3D_THREADS; }\n"
                   "typedef char gsr_filter3d_record_is_80_bytes[sizeof(gsr_filter3d_camera) == 4 * GSR_FILTER3D_CAMERA_FLOATS ? 1 : -1];\n")
    r = subprocess.run([compiler, std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_every_declared_symbol_is_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr)))
    assert names == NAMES, names
    L = _lib()
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/gsr_filter3d.h but not exported"


def test_scratch_size_is_zero_for_invalid_sizes_and_grows():
    L = _lib()
    for P in (0, -1, -(1 << 20), 1 << 30, (1 << 31) - 1):   # 3 P beyond 32-bit indexing
        assert L.gsr_filter3d_scratch_bytes(P) == 0, P
    prev = 0
    for P in (1, 2, 256, 257, 5000, 1 << 20, 6 << 20, 715827882):
        b = L.gsr_filter3d_scratch_bytes(P)
        assert b > 0 and b % 16 == 0 and b >= prev and b >= 4 * (2 + math.ceil(P / 256)), (P, b)
        prev = b


def test_entry_points_validate_before_any_device_work():
    L = _lib()
    one = 4096   # a non-NULL address that must never be dereferenced

    def compute(P=100, C=3, xyz=one, cameras=one, filt=one, scratch=one):
        return L.gsr_filter3d_compute(P, C, xyz, cameras, 0, filt, scratch, None)

    for kw in (dict(P=0), dict(P=-3), dict(P=1 << 30), dict(C=0), dict(C=-1), dict(xyz=None), dict(cameras=None), dict(filt=None), dict(scratch=None)):
        assert compute(**kw) == INVALID, kw
        assert L.gsr_last_error().startswith(b"gsr_filter3d_compute:"), (kw, L.gsr_last_error())

    for name in ("gsr_filter3d_activate", "gsr_filter3d_bake"):
        def forward(P=100, opacity=one, scaling=one, filt=one, out_o=one, out_s=one):
            return getattr(L, name)(P, opacity, scaling, filt, out_o, out_s, None)

        for kw in (dict(P=0), dict(P=-1), dict(P=1 << 30), dict(opacity=None), dict(scaling=None), dict(filt=None), dict(out_o=None, out_s=None)):
            assert forward(**kw) == INVALID, (name, kw)
            assert L.gsr_last_error().startswith(name.encode() + b":"), (kw, L.gsr_last_error())

    def backward(P=100, opacity=one, scaling=one, filt=one, d_o=one, d_s=one):
        return L.gsr_filter3d_activate_backward(P, opacity, scaling, filt, None, None, d_o, d_s, None)

    for kw in (dict(P=0), dict(P=-1), dict(P=1 << 30), dict(opacity=None), dict(scaling=None), dict(filt=None), dict(d_o=None, d_s=None)):
        assert backward(**kw) == INVALID, kw
        assert L.gsr_last_error().startswith(b"gsr_filter3d_activate_backward:"), (kw, L.gsr_last_error())

    def reset(P=100, opacity=one, scaling=one, filt=one, cap=0.01, m=one, v=one):
        return L.gsr_filter3d_reset_opacity(P, opacity, scaling, filt, cap, m, v, None)

    for kw in (dict(P=0), dict(P=-1), dict(P=1 << 30), dict(opacity=None), dict(scaling=None), dict(filt=None), dict(m=None), dict(v=None),
               dict(cap=0.0), dict(cap=1.0), dict(cap=-0.5), dict(cap=1.5), dict(cap=float("nan"))):
        assert reset(**kw) == INVALID, kw
        assert L.gsr_last_error().startswith(b"gsr_filter3d_reset_opacity:"), (kw, L.gsr_last_error())


def _dress(t):
    """a CPU tensor whose `device` attribute says cuda:0: for the checks that lie behind the device check and touch no device"""
    cuda = torch.device("cuda", 0)

    class T(torch.Tensor):
        @property
        def device(self):
            return cuda
    return t.as_subclass(T)


def test_python_surfaces_refuse_before_the_library_loads():
    import fused_filter3d as ff
    import gaussian_renderer
    from diff_gaussian_rasterization import _C, CameraModel
    from fused_params import FusedAdam
    loaded = _C._lib
    _C._lib = None
    try:
        P = 10
        opacity, scaling, f = ref.make_leaves(P, seed=1)
        xyz, cams = ref.sweep_scene(P, 2)
        rec = ff.pack_cameras(cams, "cpu")
        for cameras in (cams, rec):
            with pytest.raises(RuntimeError, match="no CPU path"):
                ff.compute_filter_3d(xyz, cameras)
        with pytest.raises(RuntimeError, match="float32"):
            ff.compute_filter_3d(xyz.double(), rec)
        for bad in (xyz[:, :2], xyz[:0], xyz.flatten()):
            with pytest.raises(RuntimeError, match=r"must be \(P, 3\)"):
                ff.compute_filter_3d(bad, rec)
        for bad in (rec[:, :19], rec[:0], rec.double(), rec[0]):
            with pytest.raises(RuntimeError, match="cameras must be"):
                ff.compute_filter_3d(xyz, bad)
        for bad in ([], None, 3):
            with pytest.raises(TypeError, match="cameras must be"):
                ff.compute_filter_3d(xyz, bad)
        with pytest.raises(TypeError, match="per_camera"):
            ff.compute_filter_3d(xyz, rec, per_camera=1)
        with pytest.raises(TypeError):
            ff.compute_filter_3d([[0.0] * 3], rec)
        fish = ref.ring_cameras(2)
        fish[1].camera_model = CameraModel("fisheye", 60.0, 60.0, 32.0, 24.0)
        with pytest.raises(NotImplementedError, match="fisheye"):
            ff.compute_filter_3d(xyz, fish)
        with pytest.raises(RuntimeError, match="is on|one device|no CPU path"):
            ff.compute_filter_3d(_dress(xyz), rec)

        for fn in (ff.filtered_activations, ff.baked_leaves, ff.activate):
            with pytest.raises(RuntimeError, match="no CPU path"):
                fn(opacity, scaling, f)
            with pytest.raises(RuntimeError, match="float32"):
                fn(opacity, scaling.double(), f)
            with pytest.raises(RuntimeError, match="float32"):
                fn(opacity, scaling, f.half())
            for o, s, ft in ((opacity[:, 0], scaling, f), (opacity, scaling[:, :2], f), (opacity, scaling, f[:, 0]), (opacity, scaling, f[:4]),
                             (opacity[:0], scaling[:0], f[:0]), (opacity, scaling, scaling)):
                with pytest.raises(RuntimeError, match=r"must be \(P, \d\)"):
                    fn(o, s, ft)
            with pytest.raises(TypeError):
                fn(opacity, scaling, 1e-3)
        with pytest.raises(ValueError, match="want"):
            ff.activate(_dress(opacity), _dress(scaling), _dress(f), want=("scales",))

        names = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
        shapes = ((P, 3), (P, 1, 3), (P, 2, 3), (P, 1), (P, 3), (P, 4))
        params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
        opt = FusedAdam([{"params": [p], "lr": 1e-3, "name": n} for p, n in zip(params, names)], lr=0.0, eps=1e-15)
        with pytest.raises(RuntimeError, match="no CPU path"):
            ff.reset_opacity(opt, f)
        for cap in (0.0, -0.01, 1.0, 2.0):
            with pytest.raises(ValueError, match="max_opacity"):
                ff.reset_opacity(opt, f, max_opacity=cap)
        with pytest.raises(RuntimeError, match=r"must be \(P, 1\)"):
            ff.reset_opacity(opt, f[:4])
        with pytest.raises(RuntimeError, match="float32"):
            ff.reset_opacity(opt, f.double())
        nameless = FusedAdam([{"params": [p], "lr": 1e-3} for p in params], lr=0.0)
        with pytest.raises(RuntimeError, match="named 'opacity'"):
            ff.reset_opacity(nameless, f)

        # render(filter_3d=): compute_cov3D_python, and a bad tensor, before anything runs
        pc = SimpleNamespace(get_xyz=torch.zeros(P, 3), _opacity=opacity, _scaling=scaling, active_sh_degree=0, max_sh_degree=0)
        cam = SimpleNamespace(image_height=8, image_width=8, FoVx=1.0, FoVy=1.0, world_view_transform=torch.eye(4), full_proj_transform=torch.eye(4),
                              camera_center=torch.zeros(3))
        pipe = SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=False)
        with pytest.raises(NotImplementedError, match="compute_cov3D_python"):
            gaussian_renderer.render(cam, pc, pipe, torch.zeros(3), filter_3d=f)
        pipe.compute_cov3D_python = False
        with pytest.raises(RuntimeError, match="no CPU path"):
            gaussian_renderer.render(cam, pc, pipe, torch.zeros(3), filter_3d=f)
        with pytest.raises(RuntimeError, match=r"must be \(P, 1\)"):
            gaussian_renderer.render(cam, pc, pipe, torch.zeros(3), filter_3d=f[:3])
        with pytest.raises(RuntimeError, match="float32"):
            gaussian_renderer.render(cam, pc, pipe, torch.zeros(3), filter_3d=f.double())
        with pytest.raises(TypeError):
            gaussian_renderer.render(cam, pc, pipe, torch.zeros(3), filter_3d=1e-3)
        assert _C._lib is None, "a refusal loaded the kernel library"
    finally:
        _C._lib = loaded


@pytest.mark.parametrize("per_camera", (False, True))
@pytest.mark.parametrize("P,C", ref.SWEEP_CASES + ((4096, 9), (20000, 33)))
def test_ambiguous_rows_of_the_gpu_scenes_stay_under_the_cap(P, C, per_camera):
    """The GPU test skips the rows whose decision lies inside the fp32 error of its own inputs.  For exactly its scenes: at most 1 % of
    the rows, never the row that holds the largest valid distance, and no open decision that could raise that distance."""
    import fused_filter3d as ff
    xyz, cams = ref.sweep_scene(P, C)
    r = ref.sweep(xyz, ff.pack_cameras(cams, "cpu"), per_camera)
    n = int(r.ambiguous.sum())
    print(f"P = {P}, C = {C}, per_camera = {per_camera}: {n} ambiguous rows, {int((~r.seen).sum())} rows valid in no camera")
    assert n <= P // 100
    assert r.dmax_row >= 0 and not bool(r.ambiguous[r.dmax_row]) and not r.risky
    assert bool(torch.isfinite(r.filter).all()) and float(r.filter.min()) > 0.0


def test_unseen_scene_has_no_valid_row_and_no_open_decision():
    import fused_filter3d as ff
    xyz, cams = ref.unseen_scene()
    r = ref.sweep(xyz, ff.pack_cameras(cams, "cpu"))
    assert not bool(r.seen.any()) and not bool(r.ambiguous.any()) and bool((r.filter == ref.UNSEEN).all())
