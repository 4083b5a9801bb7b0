"""CPU: the camera models (include/gsr_camera_model.h) without a device.  The float64 helper tests/torch_splat_camera_model.py checks
itself (analytic Jacobians against autograd, the near-axis series against the closed forms at the switch); the C header compiles as
C99 and C++17 beside gsr.h and when included twice, every function it declares is exported, and every entry point validates its
arguments before any device work; the Python surfaces refuse what has no camera-model form before the library is loaded; and the
conditions that the scenes of tests/test_camera_model_gpu.py must meet are asserted from the helper alone."""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import torch_splat_camera_model as tcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsr_camera_model.h")
LIB = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "libgsr_hip.so")
INVALID = -1   # GSR_ERR_INVALID_ARGUMENT
NAMES = ["gsr_backward_gaussians_cm", "gsr_forward_preprocess_cm", "gsr_forward_preprocess_leaf_cm"]


# ---- the helper checks itself -----------------------------------------------------------------------------------------------------
def _points():
    """view-space points: on the optical axis, r / z = 1e-4, in the series' range (q = 0.04: its truncation, q^11, is below float64's
    resolution there) and just beyond the switch (q = 0.1025), mid field, theta = 80 degrees"""
    z = 1.7
    r80 = z * math.tan(math.radians(80.0))
    return torch.tensor([[0.0, 0.0, 2.0], [0.6e-4 * z, -0.8e-4 * z, z], [0.2 * z, 0.0, z], [0.2 * z, -0.25 * z, z],
                         [0.5, 0.7, 1.1], [-1.3, 0.4, 0.9], [0.6 * r80, -0.8 * r80, z], [r80, 0.0, z]], dtype=torch.float64)


@pytest.mark.parametrize("cm", [("fisheye", 14.0, 13.0, 20.4, 11.7), ("pinhole", 35.0, 33.0, 17.3, 14.1)])
def test_analytic_jacobian_equals_autograd_of_the_projection(cm):
    pts = _points()
    W, H = 4000, 4000   # (a band wide enough that no point is clamped: the clamp is a constant by convention, not a derivative)
    if cm[0] == "pinhole":
        cm = (cm[0], cm[1], cm[2], 2000.0, 2000.0)
    _, J, inb = tcm.project(cm, pts, W, H)
    assert bool(inb.all())
    for i in range(pts.shape[0]):
        Ja = torch.autograd.functional.jacobian(lambda t: tcm.project(cm, t[None], W, H)[0][0], pts[i])
        err = float((Ja - J[i]).abs().max())
        assert err <= 1e-12 * float(J[i].abs().max()), (cm[0], i, err, J[i], Ja)
    theta = torch.atan2(pts[:, :2].norm(dim=1), pts[:, 2])
    assert float(theta.max()) > math.radians(79.9) and float(theta.min()) == 0.0


def test_fisheye_is_equidistant():
    pts = _points()
    cm = ("fisheye", 14.0, 14.0, 20.4, 11.7)
    pix, _, _ = tcm.project(cm, pts, 40, 24)
    r_pix = (pix - torch.tensor([20.4 - 0.5, 11.7 - 0.5], dtype=torch.float64)).norm(dim=1)
    theta = torch.atan2(pts[:, :2].norm(dim=1), pts[:, 2])
    assert float((r_pix - 14.0 * theta).abs().max()) < 1e-12


def test_default_intrinsics_give_the_symmetric_guard_band():
    W, H, tx, ty = 40, 24, 0.5463, 0.3278
    _, fx, fy, cx, cy = tcm.default_model(W, H, tx, ty)
    (lox, hix), (loy, hiy) = tcm.band(fx, cx, W), tcm.band(fy, cy, H)
    for v, want in ((lox, -1.3 * tx), (hix, 1.3 * tx), (loy, -1.3 * ty), (hiy, 1.3 * ty)):
        assert abs(v - want) < 1e-15


def test_series_and_closed_forms_meet_at_the_switch():
    """For every series used (s, A and dA/d(r^2)): the step between the two forms at the switch q = SERIES_Q -- the value just below
    (series) against the value just above (closed form), both at the switch itself in float64 -- is no larger than the distance
    between the helper's float32 and float64 values there."""
    q0 = tcm.SERIES_Q
    for z in (0.35, 1.0, 3.7):
        for ang in (0.0, 0.7, 2.1, 4.0):
            r = z * math.sqrt(q0)
            x, y, zz = (torch.tensor([v], dtype=torch.float64) for v in (r * math.cos(ang), r * math.sin(ang), z))
            below = tcm.fisheye_terms(x, y, zz, "series")
            above = tcm.fisheye_terms(x, y, zz, "closed")
            f32 = tcm.fisheye_terms(x.float(), y.float(), zz.float(), "closed")
            for name, b, a, f in zip(("s", "A", "Ar2"), below, above, f32):
                step, dist = abs(float(b - a)), abs(float(f.double() - a))
                print(f"{name} z={z} ang={ang}: step {step:.3e} float32 distance {dist:.3e} value {float(a):.3e}")
                assert step <= dist, (name, z, ang, step, dist)
            # and literally either side of it: one part in 1e9 below and above
            lo = tcm.fisheye_terms(x * (1 - 1e-9), y * (1 - 1e-9), zz)
            hi = tcm.fisheye_terms(x * (1 + 1e-9), y * (1 + 1e-9), zz)
            for name, b, a, f in zip(("s", "A", "Ar2"), lo, hi, f32):
                assert abs(float(b - a)) <= abs(float(f.double() - above[("s", "A", "Ar2").index(name)])) + 1e-8 * abs(float(a)), name


def test_series_coefficients():
    q = torch.tensor([0.0], dtype=torch.float64)
    assert float(tcm.series(q, "s")) == 1.0 and float(tcm.series(q, "A")) == -2.0 / 3.0 and float(tcm.series(q, "Ar2")) == 4.0 / 5.0
    # against the closed forms well inside the series' range, in float64
    x, y, z = (torch.tensor([v], dtype=torch.float64) for v in (0.11, -0.07, 1.3))
    for b, a in zip(tcm.fisheye_terms(x, y, z, "series"), tcm.fisheye_terms(x, y, z, "closed")):
        assert abs(float(b - a)) <= 1e-9 * abs(float(a))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def _lib():
    if not os.path.exists(LIB):
        __graft_entry__.build()
    from diff_gaussian_rasterization import _C
    L = ctypes.CDLL(LIB)
    L.gsr_last_error.restype = ctypes.c_char_p
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    pm, pa = ctypes.POINTER(_C.CameraModelArgs), ctypes.POINTER(_C.AuxArgs)
    pre = [i] * 5 + [vp] * 5 + [f] + [vp] * 5 + [f, f, i, vp, vp, ctypes.POINTER(ctypes.c_int64), vp, i]
    leaf = [i] * 5 + [vp] * 5 + [f] + [vp] * 4 + [f, f, i, vp, vp, ctypes.POINTER(ctypes.c_int64), vp, i]
    L.gsr_forward_preprocess_cm.restype = i
    L.gsr_forward_preprocess_cm.argtypes = [pm, i, pa] + pre
    L.gsr_forward_preprocess_leaf_cm.restype = i
    L.gsr_forward_preprocess_leaf_cm.argtypes = [pm, i, pa] + leaf
    L.gsr_backward_gaussians_cm.restype = i
    L.gsr_backward_gaussians_cm.argtypes = [ctypes.POINTER(_C.BackwardArgs), pm, i, vp, pa, i, i, i]
    return L, _C


def _declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr)))


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_alongside_the_core_abi(tmp_path, compiler, std, ext):
    src = tmp_path / f"includer.{ext}"
    src.write_text('#include "gsr.h"\n#include "gsr_camera_model.h"\n#include "gsr_camera_model.h"\n'
                   "int gsr_camera_model_includer(void) { gsr_camera_model m; m.model = GSR_CAMERA_FISHEYE; m.fx = m.fy = 1.0f; "
                   "m.cx = m.cy = 0.0f; return (int)(sizeof(&gsr_forward_preprocess_cm) + sizeof(&gsr_forward_preprocess_leaf_cm) + "
                   "sizeof(&gsr_backward_gaussians_cm) + sizeof(gsr_backward_args) + sizeof(m)) + m.model + GSR_CAMERA_PINHOLE; }\n")
    r = subprocess.run([compiler, std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_every_declared_symbol_is_exported():
    names = _declared()
    assert names == NAMES, names
    L, _ = _lib()
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/gsr_camera_model.h but not exported"


def test_struct_layout_matches_the_binding():
    _, _C = _lib()
    assert ctypes.sizeof(_C.CameraModelArgs) == 20
    assert [n for n, _ in _C.CameraModelArgs._fields_] == ["model", "fx", "fy", "cx", "cy"]
    hdr = open(HDR).read()
    for name, value in _C.CAMERA_MODELS.items():
        assert re.search(r"#define\s+GSR_CAMERA_%s\s+%d\b" % (name.upper(), value), hdr), name


BAD_MODELS = [dict(model=2), dict(model=-1), dict(fx=0.0), dict(fy=-3.0), dict(fx=float("inf")), dict(fy=float("nan")),
              dict(cx=float("nan")), dict(cy=float("-inf"))]


def _model(_C, model=1, fx=14.0, fy=14.0, cx=20.0, cy=12.0):
    return _C.CameraModelArgs(model, fx, fy, cx, cy)


@pytest.mark.parametrize("leaf", [False, True])
def test_forward_validates_before_any_device_work(leaf):
    L, _C = _lib()
    one = ctypes.c_void_p(4096)   # a non-NULL, 16-byte aligned address that must never be dereferenced
    name = "gsr_forward_preprocess_leaf_cm" if leaf else "gsr_forward_preprocess_cm"
    fn = getattr(L, name)
    R = ctypes.c_int64(7)

    def call(m, P=4, W=32, H=16, geom=one, aa=0, aux=None, rp=True):
        tail = (1.0, 1.0, 0, one, geom, ctypes.byref(R) if rp else None, None, 0)
        m = None if m is None else ctypes.byref(m)
        if leaf:
            return fn(m, aa, aux, P, 0, 1, W, H, one, one, None, one, one, 1.0, one, one, None, one, *tail)
        return fn(m, aa, aux, P, 0, 1, W, H, one, one, None, one, one, 1.0, one, None, one, None, one, *tail)

    for kw in BAD_MODELS:
        assert call(_model(_C, **kw)) == INVALID, kw
        assert L.gsr_last_error().startswith(name.encode() + b":"), (kw, L.gsr_last_error())
    for kw in (dict(P=-1), dict(W=0), dict(H=-3), dict(geom=None), dict(aa=2)):
        assert call(_model(_C), **kw) == INVALID, kw
        assert L.gsr_last_error().startswith(name.encode() + b":"), (kw, L.gsr_last_error())
    x = _C.AuxArgs()
    x.mode = 7
    assert call(_model(_C), aux=ctypes.byref(x)) == INVALID and L.gsr_last_error().startswith(name.encode() + b":")
    assert call(_model(_C), rp=False) == INVALID   # (the shared stage-1 check: no device work either)
    # nothing to do: GSR_OK with no launch, with either model and without a projection matrix
    for model in (0, 1):
        R.value = 7
        assert call(_model(_C, model=model), P=0, geom=None) == 0 and R.value == 0
        assert L.gsr_last_error() == b""
    # a NULL model is the *_aa call, with that call's validation
    assert call(None, P=0, geom=None) == 0
    assert call(None, P=-1) == INVALID and not L.gsr_last_error().startswith(name.encode())
    assert call(None, aa=2) == INVALID and L.gsr_last_error().startswith(name.replace("_cm", "_aa").encode() + b":")


def test_backward_validates_before_any_device_work():
    L, _C = _lib()
    one, name = 4096, b"gsr_backward_gaussians_cm:"

    def call(m, P=4, R=8, W=32, H=16, geom=one, args=True, aa=0, opac=None, first=0, count=4):
        a = _C.BackwardArgs()
        a.P, a.num_rendered, a.width, a.height = P, R, W, H
        a.geometry = geom
        return L.gsr_backward_gaussians_cm(ctypes.byref(a) if args else None, None if m is None else ctypes.byref(m), aa, opac, None,
                                           first, count, 0)

    for kw in BAD_MODELS:
        assert call(_model(_C, **kw)) == INVALID, kw
        assert L.gsr_last_error().startswith(name), (kw, L.gsr_last_error())
    for kw in (dict(args=False), dict(P=-1), dict(R=-1), dict(W=0), dict(H=-3), dict(geom=None), dict(aa=3), dict(aa=1, opac=None)):
        assert call(_model(_C), **kw) == INVALID, kw
        assert L.gsr_last_error().startswith(name), (kw, L.gsr_last_error())
    # every other pointer is NULL here: refused by the shared check of the per-Gaussian stage, still before any device work
    assert call(_model(_C)) == INVALID
    # nothing to do
    assert call(_model(_C), P=0, geom=None, count=0) == 0 and L.gsr_last_error() == b""
    # a NULL model is gsr_backward_gaussians_aa, with that call's validation
    assert call(None, P=0, geom=None, count=0) == 0
    assert call(None, aa=3) == INVALID and L.gsr_last_error().startswith(b"gsr_backward_gaussians_aa:")


# ---- the Python surfaces ------------------------------------------------------------------------------------------------------------
def test_python_surfaces_refuse_before_anything_runs():
    import diff_gaussian_rasterization as dgr
    import fused_params
    import gaussian_renderer
    import view_parallel
    from diff_gaussian_rasterization import _C
    loaded = _C._lib
    _C._lib = None
    try:
        s = dgr.GaussianRasterizationSettings(16, 16, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                              torch.zeros(3), False, False)
        m = torch.zeros(4, 3)
        good = dgr.CameraModel("fisheye", 10.0, 10.0, 8.0, 8.0)
        module = lambda **kw: dgr.GaussianRasterizer(s, **kw)
        leaf = lambda **kw: fused_params.rasterize_leaf_gaussians(m, m, torch.zeros(4, 1, 3), torch.zeros(4, 0, 3), torch.zeros(4, 1), m,
                                                                  torch.zeros(4, 4), s, **kw)
        function = lambda **kw: dgr.rasterize_gaussians_depth_alpha(
            m, m, torch.zeros(4, 1, 3), torch.Tensor([]), torch.zeros(4, 1), m, torch.zeros(4, 4), torch.Tensor([]), s, "depth", **kw)
        plain = lambda **kw: dgr.rasterize_gaussians(m, m, torch.zeros(4, 1, 3), torch.Tensor([]), torch.zeros(4, 1), m, torch.zeros(4, 4),
                                                     torch.Tensor([]), s, **kw)
        direct = lambda camera_model=None, camera_grads=False: _C.camera_model_excludes(_C.camera_model(camera_model), camera_grads)

        class Pipe:
            compute_cov3D_python = convert_SHs_python = debug = False

        class PC:
            active_sh_degree = 0
            get_xyz = m

        class Cam:
            image_width = image_height = 16
            FoVx = FoVy = 1.0
            world_view_transform = full_proj_transform = torch.eye(4)
            camera_center = torch.zeros(3)

        renderer = lambda **kw: gaussian_renderer.render(Cam(), PC(), Pipe(), torch.zeros(3), **kw)
        surfaces = (direct, module, leaf, function, plain, renderer)
        for surface in surfaces:
            for bad in (3, "fisheye", ("pinhole", 1.0, 1.0, 1.0), ["pinhole", 1.0, 1.0, 1.0, 1.0], (0, 1.0, 1.0, 1.0, 1.0),
                        ("pinhole", "1", 1.0, 1.0, 1.0), ("pinhole", 1.0, 1.0, 1.0, True), torch.ones(5)):
                with pytest.raises(TypeError, match="camera_model"):
                    surface(camera_model=bad)
            for bad in (("orthographic", 1.0, 1.0, 1.0, 1.0), ("Pinhole", 1.0, 1.0, 1.0, 1.0), ("fisheye", 0.0, 1.0, 1.0, 1.0),
                        ("fisheye", 1.0, -2.0, 1.0, 1.0), ("pinhole", float("inf"), 1.0, 1.0, 1.0), ("pinhole", 1.0, 1.0, float("nan"), 1.0)):
                with pytest.raises(ValueError, match="camera_model"):
                    surface(camera_model=bad)
            with pytest.raises(NotImplementedError, match="camera_grads"):
                surface(camera_model=good, camera_grads=True)
            with pytest.raises(NotImplementedError, match="camera_grads"):
                surface(camera_model=tuple(good), camera_grads=True)
        # the camera's own attribute is picked up by render() when the keyword is None
        class FisheyeCam(Cam):
            camera_model = ("orthographic", 1.0, 1.0, 1.0, 1.0)
        with pytest.raises(ValueError, match="camera_model"):
            gaussian_renderer.render(FisheyeCam(), PC(), Pipe(), torch.zeros(3))
        assert module(camera_model=good).camera_model == good and module(camera_model=tuple(good)).camera_model == good
        assert module().camera_model is None
        assert isinstance(module(camera_model=("pinhole", 3, 4, 5, 6)).camera_model.fx, float)
        # ---- out of scope: the view-parallel paths
        with pytest.raises(NotImplementedError, match="camera_model"):
            view_parallel.rasterize_view_parallel(m, m, torch.zeros(4, 1, 3), torch.zeros(4, 1), m, torch.zeros(4, 4), s, None,
                                                  camera_model=good)
        with pytest.raises(NotImplementedError, match="camera_model"):
            view_parallel.ViewsInFlight.forward_backward(None, [], [], camera_model=good)
        assert _C._lib is None, "a refusal loaded the kernel library"
    finally:
        _C._lib = loaded


# ---- the conditions of the GPU scenes, from the helper alone ------------------------------------------------------------------------
def _state(cm, scene, cam, W=None, H=None, variant="sh", **kw):
    W, H = W or cam.image_width, H or cam.image_height
    inp = tcm.scene_inputs(scene, cam, variant)
    with torch.no_grad():
        out = tcm.render(cm, W, H, scene.bg, 3, V=inp.pop("V"), campos=inp.pop("campos"), **inp, **kw)
    return out["state"]


def _caps(st):
    assert float(st["fragile"].double().mean()) <= 0.10, "more than 10 % of the pixels are fragile"
    assert float(st["fragile_radius"].double().mean()) <= 0.01, "more than 1 % of the Gaussians have a fragile radius"


def test_gpu_scene_conditions_default_and_offcentre():
    scene, cam = tcm.base_scene()
    W, H = cam.image_width, cam.image_height
    for cm in (tcm.default_model(W, H, cam.tanfovx, cam.tanfovy), tcm.PINHOLE_OFFCENTRE):
        for kw in ({}, dict(antialiasing=True)):
            st = _state(cm, scene, cam, **kw)
            _caps(st)
            assert int((~st["vis"]).sum()) >= 10 and int(st["vis"].sum()) >= 200
    for shape in tcm.EDGE_SHAPES:
        scene, cam = tcm.base_scene(300, *shape)
        _caps(_state(tcm.default_model(*shape, cam.tanfovx, cam.tanfovy), scene, cam))


def test_gpu_scene_conditions_crop():
    scene, cam, (W, H), (x0, y0), cm = tcm.crop_scene()
    assert x0 % 16 == 0 and y0 % 16 == 0 and cm[3] != W / 2 and cm[4] != H / 2
    big = _state(tcm.default_model(cam.image_width, cam.image_height, cam.tanfovx, cam.tanfovy), scene, cam)
    small = _state(cm, scene, cam, W, H)
    _caps(small)
    assert float(big["fragile"][y0:y0 + H, x0:x0 + W].double().mean()) <= 0.10
    vis = small["vis"]
    assert int(vis.sum()) >= 50
    assert bool(small["in_band"][vis].all()) and bool(big["in_band"][vis].all()), "a Gaussian of the crop sits in a guard band"
    # the crop's Gaussians have the same radius in both renders and the same tiles, shifted
    assert bool((small["radii"][vis] == big["radii"][vis]).all())


def test_gpu_scene_conditions_guard_band():
    scene, cam, cm, k = tcm.guard_scene()
    W, H = cam.image_width, cam.image_height
    st = _state(cm, scene, cam)
    _caps(st)
    txtz = st["t"][:, 0] / st["t"][:, 2]
    old = 1.3 * cam.tanfovx
    _, new = tcm.band(cm[1], cm[3], W)
    between = st["vis"] & (txtz > old) & (txtz < new)
    assert int(between.sum()) >= 5 and bool(between[k].all()), int(between.sum())
    assert bool(st["in_band"][between].all())


def test_gpu_scene_conditions_fisheye():
    scene, cam, cm = tcm.fisheye_scene()
    W, H = cam.image_width, cam.image_height
    for variant, kw in (("sh", {}), ("sh", dict(antialiasing=True)), ("colors", {}), ("cov", {})):
        st = _state(cm, scene, cam, variant=variant, **kw)
        _caps(st)
    t, vis = st["t"], st["vis"]
    r = t[:, :2].norm(dim=1)
    assert float(r[24]) == 0.0 and bool(vis[24]), "no visible Gaussian exactly on the optical axis"
    q = (r / t[:, 2]) ** 2
    assert bool(vis[25]) and 0.0 < float(q[25]) < tcm.SERIES_Q
    theta = torch.atan2(r, t[:, 2])
    assert bool(vis[26]) and float(theta[26]) > math.radians(75.0)
    assert int((vis & (q >= tcm.SERIES_Q)).sum()) >= 20 and int((vis & (q < tcm.SERIES_Q)).sum()) >= 20   # both forms are exercised
    assert int((~vis).sum()) >= 10


def test_gpu_scene_conditions_oracle_pin():
    scene, cam, cm = tcm.oracle_pin_scene()
    W, H = cam.image_width, cam.image_height
    st = _state(cm, scene, cam, variant="colors")
    _caps(st)
    t, vis = st["t"], st["vis"]
    r = t[:, :2].norm(dim=1)
    assert bool(vis[24]) and float(r[24]) == 0.0 and bool(vis[26]) and float(torch.atan2(r[26], t[26, 2])) > math.radians(75.0)
    assert int(vis.sum()) >= 200 and int((~vis).sum()) >= 10
    # no visible stand-in inside the core camera's guard band clamp: the oracle's Jacobian of the stand-in is then the plain pinhole's
    S = tcm.covariance3d(scene.scales.double(), scene.rotations.double(), 1.0, None)
    _, _, in_core = tcm.pinhole_standin(cm, W, H, cam.tanfovx, cam.tanfovy, scene.means3D, cam.world_view_transform, S)
    assert bool(in_core[vis].all()), "a visible stand-in sits in the oracle's guard band"
