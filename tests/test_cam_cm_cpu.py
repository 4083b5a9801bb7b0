"""CPU: camera gradients under a camera model (include/gsr_cam_cm.h, `camera_model_grads=`) without a device.  The float64 helper
tests/torch_splat_cam_cm.py is the function of tests/torch_splat_camera_model.py when given the same camera; the closed-form terms of
DESIGN 6o equal its autograd per Gaussian; two reference-free identities hold on it; the scenes of tests/test_cam_cm_gpu.py meet
their conditions; the C header compiles as C99, the library exports the two new names and validates before any device work; and the
Python surfaces refuse what they must before the library is loaded."""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import torch_splat_cam_cm as tcc
import torch_splat_camera_model as tcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsr_cam_cm.h")
PKG = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd")
LIB = os.path.join(PKG, "libgsr_hip.so")
INVALID = -1   # GSR_ERR_INVALID_ARGUMENT
NAMES = ["gsr_backward_gaussians_cam_cm", "gsr_cam_cm_bytes"]


def _caps(st):
    assert float(st["fragile"].double().mean()) <= 0.10, "more than 10 % of the pixels are fragile"
    assert float(st["fragile_radius"].double().mean()) <= 0.01, "more than 1 % of the Gaussians have a fragile radius"


def _dL(st, H, W, depth_mode, seed=1):
    dL = {"image": tcm.fragile_free(st, (3, H, W), seed)}
    if depth_mode is not None:
        dL["depth"], dL["alpha"] = tcm.fragile_free(st, (H, W), seed + 1), tcm.fragile_free(st, (H, W), seed + 2)
    return dL


# ---- the helper equals the existing one ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["pinhole", "fisheye"])
@pytest.mark.parametrize("variant,kw", [("sh", {}), ("sh", dict(antialiasing=True)), ("sh", dict(depth_mode="invdepth"))])
def test_helper_equals_the_camera_model_helper(which, variant, kw):
    if which == "pinhole":
        scene, cam, cm, _ = tcm.guard_scene()
    else:
        scene, cam, cm = tcm.fisheye_scene()
    W, H = cam.image_width, cam.image_height
    inp = tcm.scene_inputs(scene, cam, variant)
    st = tcc.probe_state(cm, W, H, scene.bg, 3, inp, **kw)
    _caps(st)
    dL = _dL(st, H, W, kw.get("depth_mode"))
    out_a, g_a = tcm.loss_and_grads(cm, W, H, scene.bg, 3, inp, dL, torch.float64, st, **kw)
    diff = {k: v.double().clone().requires_grad_(True) for k, v in inp.items() if k not in ("V", "campos")}
    out_b = tcc.render(cm[0], W, H, scene.bg, 3, st, V=inp["V"], campos=inp["campos"], K=tcc.intrinsics(cm), **diff, **kw)
    grads = torch.autograd.grad(tcc._loss(out_b, dL, torch.float64), list(diff.values()), allow_unused=True)
    for k in dL:
        assert float((out_a[k] - out_b[k]).detach().abs().max()) <= 1e-12 * max(1.0, float(out_a[k].detach().abs().max())), k
    for (k, v), g in zip(diff.items(), grads):
        g = torch.zeros_like(v) if g is None else g
        assert float((g - g_a[k]).abs().max()) <= 1e-12 * max(1.0, float(g_a[k].abs().max())), k


# ---- closed forms against autograd, per Gaussian ---------------------------------------------------------------------------------------
def _closed_forms_case(scene, cam, cm, kw):
    W, H = cam.image_width, cam.image_height
    inp = tcm.scene_inputs(scene, cam, "sh")
    st = tcc.probe_state(cm, W, H, scene.bg, 3, inp, **kw)
    _caps(st)
    dL = _dL(st, H, W, kw.get("depth_mode"))
    P = scene.means3D.shape[0]
    camt = {"V": inp["V"].double().expand(P, 4, 4).clone().requires_grad_(True),
            "campos": inp["campos"].double().expand(P, 3).clone().requires_grad_(True),
            "K": tcc.intrinsics(cm).expand(P, 4).clone().requires_grad_(True)}
    g = {k: v.double().clone().requires_grad_(True) for k, v in inp.items() if k not in camt}
    keep = {}
    out = tcc.render(cm[0], W, H, scene.bg, 3, st, dtype=torch.float64, keep=keep, **camt, **g, **kw)
    tcc._loss(out, dL, torch.float64).backward()
    closed = tcc.closed_forms(cm, W, H, keep, scene.means3D)
    worst = 0.0
    for k in ("V", "campos", "K"):
        auto = camt[k].grad
        scale = auto.reshape(P, -1).abs().max(1).values
        err = (closed[k] - auto).reshape(P, -1).abs().max(1).values
        assert bool((err <= 1e-10 * scale).all()), (k, int((err > 1e-10 * scale).sum()), float((err / scale.clamp_min(1e-300)).max()))
        worst = max(worst, float((err / scale.clamp_min(1e-300))[scale > 0].max()))
        assert bool((auto[:, :, 3] == 0).all()) if k == "V" else True
    print(f"closed forms vs autograd, {cm[0]}: worst relative error per Gaussian {worst:.2e}")
    return st, {k: v.grad for k, v in camt.items()}


@pytest.mark.parametrize("kw", [{}, dict(antialiasing=True, depth_mode="invdepth")])
def test_closed_forms_equal_autograd_fisheye(kw):
    scene, cam, cm, idx = tcc.fisheye_points_scene()
    st, terms = _closed_forms_case(scene, cam, cm, kw)
    t, vis = st["t"], st["vis"]
    r = t[:, :2].norm(dim=1)
    q = (r / t[:, 2]) ** 2
    live = lambda i: bool(vis[i]) and float(terms["K"][i].abs().max()) > 0 and float(terms["V"][i].abs().max()) > 0
    assert float(r[idx["axis"]]) == 0.0 and live(idx["axis"])
    assert abs(float(r[idx["near_axis"]] / t[idx["near_axis"], 2]) - 1e-4) < 1e-9 and live(idx["near_axis"])
    assert abs(math.degrees(float(torch.atan2(r[idx["wide"]], t[idx["wide"], 2]))) - 80.0) < 1e-3 and live(idx["wide"])
    assert 0.0995 < float(q[idx["below"]]) < tcm.SERIES_Q < float(q[idx["above"]]) < 0.1005 and live(idx["below"]) and live(idx["above"])


@pytest.mark.parametrize("kw", [{}, dict(antialiasing=True, depth_mode="depth")])
def test_closed_forms_equal_autograd_in_the_guard_band(kw):
    scene, cam, cm, idx = tcc.guard_sides_scene()
    st, terms = _closed_forms_case(scene, cam, cm, kw)
    W = cam.image_width
    txtz = st["t"][:, 0] / st["t"][:, 2]
    lox, hix = tcm.band(cm[1], cm[3], W)
    live = lambda i: bool(st["vis"][i]) and float(terms["K"][i].abs().max()) > 0
    inside = [int(i) for i in idx["inside"]]
    assert all(1.3 * cam.tanfovx < float(txtz[i]) < hix and bool(st["in_band"][i]) for i in inside) and sum(live(i) for i in inside) >= 3
    assert all(float(txtz[i]) > hix and not bool(st["in_band"][i]) for i in idx["beyond_hi"]) and sum(live(int(i)) for i in idx["beyond_hi"]) >= 2
    assert all(float(txtz[i]) < lox and not bool(st["in_band"][i]) for i in idx["beyond_lo"]) and sum(live(int(i)) for i in idx["beyond_lo"]) >= 2


# ---- reference-free identities on the helper ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["pinhole", "fisheye"])
def test_shift_and_principal_point_identities_on_the_helper(which):
    """Translating the world by delta is the same function as shifting the camera: sum_g dL/dmean_g[k] = sum_i dL/dV[12+i] V[4k+i] -
    dL/dcampos[k]; and moving the principal point moves every pixel mean: dL/dcx = sum_g means2D.grad[g, 0] / (0.5 W)."""
    if which == "pinhole":
        scene, cam, cm, _ = tcm.guard_scene()
    else:
        scene, cam, cm = tcm.fisheye_scene()
    W, H = cam.image_width, cam.image_height
    inp = tcm.scene_inputs(scene, cam, "sh")
    st = tcc.probe_state(cm, W, H, scene.bg, 3, inp)
    _caps(st)
    dL = _dL(st, H, W, None)
    total, abs_total, _, gg, _ = tcc.camera_terms(cm, W, H, scene.bg, 3, inp, dL, st, want_gaussians=True)
    V = inp["V"].double()
    for k in range(3):
        lhs = float(gg["means3D"][:, k].sum())
        rhs = float(sum(total["V"][3, i] * V[k, i] for i in range(3)) - total["campos"][k])
        assert abs(lhs - rhs) <= 1e-12 * float(gg["means3D"][:, k].abs().sum()), (k, lhs, rhs)
    for j, S in ((0, W), (1, H)):
        lhs, rhs = float(total["K"][2 + j]), float(gg["means2D"][:, j].sum() / (0.5 * S))
        assert abs(lhs - rhs) <= 1e-12 * float(gg["means2D"][:, j].abs().sum() / (0.5 * S)), (j, lhs, rhs)
    assert float(total["K"].abs().min()) > 0 and float(total["campos"].abs().min()) > 0


# ---- the conditions of the GPU scenes -----------------------------------------------------------------------------------------------------
def test_gpu_scene_conditions():
    for maker, variants in ((lambda: tcm.base_scene() + (tcm.default_model(40, 24, *_tan(tcm.base_scene()[1])),), ("sh",)),
                            (lambda: tcm.guard_scene()[:3], ("sh", "colors", "cov")),
                            (lambda: tcm.fisheye_scene(), ("sh", "colors", "cov")),
                            (lambda: tcm.base_scene(300, 37, 21) + (("pinhole", 33.0, 31.0, 12.3, 13.9),), ("sh",))):
        scene, cam, cm = maker()
        for variant in variants:
            for kw in ({}, dict(antialiasing=True)):
                inp = tcm.scene_inputs(scene, cam, variant)
                st = tcc.probe_state(cm, cam.image_width, cam.image_height, scene.bg, 3, inp, **kw)
                _caps(st)
                assert int((~st["vis"]).sum()) >= 10 and int(st["vis"].sum()) >= 200


def _tan(cam):
    return cam.tanfovx, cam.tanfovy


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def _lib():
    if not os.path.exists(LIB):
        __graft_entry__.build()
    from diff_gaussian_rasterization import _C
    return _C.lib(), _C


def test_header_compiles_as_c99_and_runs(tmp_path):
    _lib()
    exe = tmp_path / "cam_cm_abi"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "cam_cm_abi.c"), "-o", str(exe), "-L" + PKG, "-lgsr_hip",
                        "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cam_cm_abi ok" in r.stdout, r.stdout + r.stderr


def test_the_library_exports_exactly_the_two_new_names():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr))) == NAMES
    L, _ = _lib()
    r = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    c_names = sorted(l.split()[-1] for l in r.stdout.splitlines() if re.search(r"\sT\s+gsr_\w*cam_cm\w*$", l))
    assert c_names == NAMES, c_names
    for n in NAMES:
        assert hasattr(L, n)


def test_scratch_size():
    L, _ = _lib()
    assert L.gsr_cam_cm_bytes(0) >= 16 and L.gsr_cam_cm_bytes(-3) >= 16
    last = 0
    for P in (-3, 0, 1, 63, 64, 65, 4097, 100_003, 1 << 20, (1 << 31) - 1):
        assert L.gsr_cam_cm_bytes(P) >= last
        last = L.gsr_cam_cm_bytes(P)
        assert last >= ((max(P, 0) + 63) // 64) * 20 * 4   # at least the 20 used floats per wave of 64 Gaussians


def _args(_C, P=128):
    """A gsr_backward_args that passes the core checks with fake (never dereferenced) addresses."""
    a = _C.BackwardArgs()
    for name, typ in a._fields_:
        if typ is ctypes.c_void_p and name not in ("stream", "colors_precomp", "cov3D_precomp", "dL_dcov3D", "dL_dconic", "shs_rest",
                                                   "dL_dsh_rest", "stat_xyz_gradient_accum", "stat_denom", "stat_max_radii2D"):
            setattr(a, name, 0x1000)
    a.P, a.D, a.M, a.num_rendered, a.width, a.height = P, 0, 1, 10, 32, 32
    a.tan_fovx = a.tan_fovy = 0.5
    a.scale_modifier = 1.0
    return a


def _cam(_C, **over):
    c = _C.CamCmArgs()
    c.dL_dviewmatrix, c.dL_dintrinsics, c.dL_dcampos, c.scratch = 0x2000, 0x3000, 0x4000, 0x5000
    for k, v in over.items():
        setattr(c, k, v)
    return c


def test_entry_point_validates_before_any_device_work():
    L, _C = _lib()
    name = b"gsr_backward_gaussians_cam_cm:"
    model = lambda **kw: _C.CameraModelArgs(**{**dict(model=1, fx=14.0, fy=14.0, cx=20.0, cy=12.0), **kw})

    def call(a=None, m=True, cam=True, first=0, count=None, aa=0, opac=None, args=True, **cam_over):
        a = _args(_C) if a is None else a
        m = model() if m is True else m
        c = _cam(_C, **cam_over) if cam is True else cam
        return L.gsr_backward_gaussians_cam_cm(ctypes.byref(a) if args else None, None if m is None else ctypes.byref(m), aa, opac, None,
                                               None if c is None else ctypes.byref(c), first, a.P if count is None else count, 0)

    def refused(**kw):
        assert call(**kw) == INVALID, kw
        assert L.gsr_last_error().startswith(name), (kw, L.gsr_last_error())

    refused(m=None)                                          # cam needs a model
    for bad in (dict(model=2), dict(fx=0.0), dict(fy=float("nan")), dict(cx=float("inf"))):
        refused(m=model(**bad))
    refused(first=64)                                        # the whole scene in one call
    refused(count=64)
    refused(first=64, count=64)
    refused(dL_dviewmatrix=None)                             # non-NULL outputs and scratch
    refused(dL_dintrinsics=None)
    refused(dL_dcampos=None)
    refused(scratch=None)
    refused(scratch=0x5004)                                  # 16-byte aligned
    refused(args=False)
    refused(aa=3)
    refused(aa=1, opac=None)
    bad = _args(_C)
    bad.width = 0
    refused(a=bad)
    bad = _args(_C)
    bad.geometry = None
    refused(a=bad)
    bad = _args(_C)
    bad.cam_pos = None
    refused(a=bad)
    # cam == NULL: gsr_backward_gaussians_cm, argument for argument, with that call's validation
    assert call(cam=None, m=model(model=2)) == INVALID and L.gsr_last_error().startswith(b"gsr_backward_gaussians_cm:")
    empty = _C.BackwardArgs()
    empty.width = empty.height = 16
    assert call(a=empty, cam=None, count=0) == 0 and L.gsr_last_error() == b""
    # ... and with neither, gsr_backward_gaussians_aa
    assert call(cam=None, m=None, aa=3) == INVALID and L.gsr_last_error().startswith(b"gsr_backward_gaussians_aa:")


def test_struct_layout_matches_the_binding():
    _, _C = _lib()
    assert ctypes.sizeof(_C.CamCmArgs) == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in _C.CamCmArgs._fields_] == ["dL_dviewmatrix", "dL_dintrinsics", "dL_dcampos", "scratch"]
    hdr = open(HDR).read()
    order = [hdr.index(n + ";") for n in ("dL_dviewmatrix", "dL_dintrinsics", "dL_dcampos", "scratch")]
    assert order == sorted(order)


# ---- the Python surfaces ----------------------------------------------------------------------------------------------------------------
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
        for surface in (module, leaf, function, plain, renderer):
            for on in (True, torch.zeros(4)):
                with pytest.raises(ValueError, match="camera_model"):     # no camera model
                    surface(camera_model_grads=on)
            for bad in (1, 0, "yes", None if surface is not renderer else 2.5, (1.0, 1.0, 1.0, 1.0), [True]):
                with pytest.raises(TypeError, match="camera_model_grads"):
                    surface(camera_model=good, camera_model_grads=bad)
            for bad in (torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.int32), torch.zeros(5), torch.zeros(1, 4),
                        torch.zeros(()), torch.zeros(4)):                  # dtype, shape, and a tensor that is not on a HIP device
                with pytest.raises(ValueError, match="camera_model_grads"):
                    surface(camera_model=good, camera_model_grads=bad)
            # the combination that existed before is still refused, and its message still names camera_grads
            with pytest.raises(NotImplementedError, match="camera_grads"):
                surface(camera_model=good, camera_grads=True)
            with pytest.raises(NotImplementedError, match="camera_grads"):
                surface(camera_model=good, camera_grads=True, camera_model_grads=True)
        # render(): None means the pipe's own attribute
        class GradPipe(Pipe):
            camera_model_grads = True
        with pytest.raises(ValueError, match="camera_model"):
            gaussian_renderer.render(Cam(), PC(), GradPipe(), torch.zeros(3))
        assert module(camera_model=good, camera_model_grads=True).camera_model_grads is True
        assert module(camera_model=good).camera_model_grads is False and module().camera_model_grads is False
        # ---- no view-parallel form, no part-by-part form
        for on in (True, torch.zeros(4)):
            with pytest.raises(NotImplementedError, match="camera_model_grads"):
                view_parallel.rasterize_view_parallel(m, m, torch.zeros(4, 1, 3), torch.zeros(4, 1), m, torch.zeros(4, 4), s, None,
                                                      camera_model=good, camera_model_grads=on)
            with pytest.raises(NotImplementedError, match="camera_model_grads"):
                view_parallel.ViewsInFlight.forward_backward(None, [], [], camera_model=good, camera_model_grads=on)
        with pytest.raises(NotImplementedError, match="parts"):
            _C.run_backward(_C.BackwardArgs(), None, None, cam=_C.CamCmArgs(), parts=((0, 64),), camera_model=good)
        assert _C._lib is None, "a refusal loaded the kernel library"
    finally:
        _C._lib = loaded


def test_camera_model_from_tensor():
    from diff_gaussian_rasterization import CameraModel
    k = torch.tensor([14.25, 13.5, 20.4, 11.7], requires_grad=True)
    cm = CameraModel.from_tensor("fisheye", k)
    assert cm == CameraModel("fisheye", *(float(v) for v in k.detach()))
    assert all(isinstance(v, float) for v in cm[1:])
    with pytest.raises(ValueError):
        CameraModel.from_tensor("fisheye", torch.zeros(5))
    with pytest.raises(ValueError):
        CameraModel.from_tensor("fisheye", torch.tensor([0.0, 1.0, 1.0, 1.0]))   # the model's own checks apply
    from diff_gaussian_rasterization import _C
    _C.camera_model_matches(cm, k)
    with pytest.raises(ValueError, match="camera_model_grads"):
        _C.camera_model_matches(cm, k.detach() + torch.tensor([0.0, 0.0, 0.5, 0.0]))
