"""CPU: the C-ABI library loads and exports every symbol include/gsr.h declares; host-only entry
points behave; the Python drop-in surface has the reference's shape.  No GPU compute is called."""
import ctypes
import os
import re

import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "libgsr_hip.so")


def _lib():
    if not os.path.exists(LIB):
        __graft_entry__.build()
    return ctypes.CDLL(LIB)


def test_every_declared_symbol_is_exported():
    hdr = open(os.path.join(ROOT, "include", "gsr.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 15, names
    L = _lib()
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/gsr.h but not exported"


def test_host_only_entry_points():
    L = _lib()
    L.gsr_version.restype = ctypes.c_char_p
    assert b"gfx950" in L.gsr_version()
    L.gsr_get_higher_msb.restype = ctypes.c_uint32
    for n in (1, 2, 255, 256, 8432, 32400, 65536):
        assert L.gsr_get_higher_msb(ctypes.c_uint32(n)) == oracle.get_higher_msb(n)
    L.gsr_geometry_bytes.restype = ctypes.c_size_t
    L.gsr_image_bytes.restype = ctypes.c_size_t
    g1, g2 = L.gsr_geometry_bytes(1000), L.gsr_geometry_bytes(2000)
    assert 48 * 1000 < g1 < g2
    assert L.gsr_image_bytes(1980, 1080) >= 8 * 1980 * 1080
    # argument validation happens before any device work
    L.gsr_last_error.restype = ctypes.c_char_p
    R = ctypes.c_int64(0)
    rc = L.gsr_forward_preprocess(-1, 0, 0, 16, 16, None, None, None, None, None, ctypes.c_float(1), None, None, None,
                                  None, None, ctypes.c_float(1), ctypes.c_float(1), 0, None, None, ctypes.byref(R), None, 0)
    assert rc == -1 and b"bad" in L.gsr_last_error()


def test_layouts_of_the_column_pair_binning():
    """Host-only: which images are binned by column pairs (at most 256 x 256 tiles), and the room the two passes need inside
    the blobs -- pass 1: per-1024-Gaussian digit rows + 16 bytes per Gaussian in the geometry blob; pass 2: one digit row per
    1024 column pairs (+ one per tile column) in the binning blob's table area; the sorted pairs (8 bytes, at most R of them)
    in point_list_alt + tile_keys."""
    from diff_gaussian_rasterization import _C
    for W, H, want in ((1980, 1080, 1), (3840, 2160, 1), (4096, 4096, 1), (4097, 16, 0), (16, 4097, 0), (1, 1, 1)):
        assert int(_C.binning_layout(10, 100, W, H).column_pairs) == want, (W, H)
    for P in (1, 1000, 1_000_000):
        gl = _C.geometry_layout(P)
        blocks = (P + 1023) // 1024
        assert gl.total - gl.col_table >= 4 * 256 * (blocks + 1) + 16 * P and gl.col_table >= gl.sort_table
    for R in (1, 5000, 9_161_997):
        bl = _C.binning_layout(1000, R, 1980, 1080)
        assert bl.checkpoints - bl.sort_table >= 4 * 256 * (R // 1024 + 256)
        assert bl.tile_keys_alt - bl.point_list_alt >= 8 * R and bl.total > bl.checkpoints


def test_python_surface_matches_reference_shape():
    import diff_gaussian_rasterization as dgr
    # reference diff_gaussian_rasterization/__init__.py:168-180
    assert dgr.GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "campos", "prefiltered", "debug")
    for name in ("GaussianRasterizer", "rasterize_gaussians", "_RasterizeGaussians", "cpu_deep_copy_tuple", "_C"):
        assert hasattr(dgr, name)
    for name in ("rasterize_gaussians", "rasterize_gaussians_backward", "mark_visible"):  # ext.cpp:18-22
        assert hasattr(dgr._C, name)
    assert issubclass(dgr.GaussianRasterizer, torch.nn.Module)


def test_validation_and_no_cpu_fallback():
    import diff_gaussian_rasterization as dgr
    s = dgr.GaussianRasterizationSettings(16, 16, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                          torch.zeros(3), False, False)
    r = dgr.GaussianRasterizer(s)
    m = torch.zeros(4, 3)
    with pytest.raises(Exception, match="Please provide excatly one of either SHs or precomputed colors!"):
        r(means3D=m, means2D=m, opacities=torch.ones(4, 1), scales=m, rotations=torch.zeros(4, 4))
    with pytest.raises(Exception, match="Please provide exactly one of either scale/rotation pair"):
        r(means3D=m, means2D=m, opacities=torch.ones(4, 1), shs=torch.zeros(4, 1, 3), cov3D_precomp=torch.zeros(4, 6),
          scales=m)
    # CPU tensors are refused loudly: the product path never falls back to the oracle or to eager PyTorch
    with pytest.raises(RuntimeError, match="no CPU path"):
        r(means3D=m, means2D=m, opacities=torch.ones(4, 1), shs=torch.zeros(4, 1, 3), scales=m, rotations=torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.markVisible(m)


def test_product_package_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dp, f)).read()
                assert "oracle" not in src.replace("the CPU oracle", "").replace("CPU oracle", "") or f in (), \
                    f"{f} mentions the oracle: the product path must not depend on it"


def test_8f_entry_points_validate_before_any_device_work():
    import fused_params
    L = _lib()
    L.gsr_last_error.restype = ctypes.c_char_p
    L.gsr_knn_scratch_bytes.restype = ctypes.c_size_t
    assert L.gsr_knn_scratch_bytes(0) == 0 and 0 < L.gsr_knn_scratch_bytes(1000) < L.gsr_knn_scratch_bytes(100000)
    assert L.gsr_knn_mean_dist2(-1, None, None, None, None) == -1
    assert L.gsr_knn_mean_dist2(10, None, None, None, None) == -1 and b"NULL" in L.gsr_last_error()
    assert L.gsr_knn_mean_dist2(0, None, None, None, None) == 0
    L.gsr_adam_step.argtypes = [ctypes.c_int, ctypes.POINTER(fused_params.AdamGroup), ctypes.c_double, ctypes.c_double,
                                ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    assert ctypes.sizeof(fused_params.AdamGroup) == 64    # include/gsr.h gsr_adam_group: 4 pointers, 2 int64, double, int32 (+pad)
    g = (fused_params.AdamGroup * 1)(fused_params.AdamGroup(None, None, None, None, 8, 0, 1e-3, 1))
    assert L.gsr_adam_step(1, g, 0.9, 0.999, 1e-15, None, None) == -1 and b"step < 1" in L.gsr_last_error()
    assert L.gsr_adam_step(9, g, 0.9, 0.999, 1e-15, None, None) == -1
    assert L.gsr_adam_step(0, None, 0.9, 0.999, 1e-15, None, None) == 0
    g[0].step, g[0].numel = 1, 0     # an empty group is a no-op, no launch
    assert L.gsr_adam_step(1, g, 0.9, 0.999, 1e-15, None, None) == 0
    R = ctypes.c_int64(0)
    f1 = ctypes.c_float(1)
    rc = L.gsr_forward_preprocess_leaf(5, 0, 1, 16, 16, None, None, None, None, None, f1, None, None, None, None, f1, f1, 0,
                                       None, None, ctypes.byref(R), None, 0)
    assert rc == -1 and b"NULL" in L.gsr_last_error()


def test_aux_and_aa_entry_points_validate_before_any_device_work():
    """include/gsr_aux.h / gsr_aa.h: what every *_aux / *_aa entry point rejects about its gsr_aux_args (and the filter's opacity
    input) before any HIP call, and that an empty scene is GSR_OK with nothing launched.  Where the remaining arguments would be
    rejected as well, P == 0 or the message's prefix tells the option's own check apart from the stage's."""
    from diff_gaussian_rasterization import _C
    L = _C.lib()
    OK, BAD = 0, -1
    err = L.gsr_last_error
    f1 = ctypes.c_float(1)
    R = ctypes.c_int64(-1)
    buf = ctypes.create_string_buffer(64 + 16)   # never dereferenced: the calls below return before any device work
    aligned = (ctypes.addressof(buf) + 15) & ~15

    def aux_args(mode=1, scratch=aligned, out=aligned):
        return _C.AuxArgs(mode, out, out, None, None, scratch)

    def pre(P=0, width=8):       # the arguments of gsr_forward_preprocess; gsr_forward_preprocess_leaf has one pointer fewer
        return [P, 0, 1, width, 8] + [None] * 5 + [f1] + [None] * 5 + [f1, f1, 0, None, None, ctypes.byref(R), None, 0]

    def pre_leaf(P=0):
        return [P, 0, 1, 8, 8] + [None] * 5 + [f1] + [None] * 4 + [f1, f1, 0, None, None, ctypes.byref(R), None, 0]

    def render(P=0):
        return [P, 0, 8, 8] + [None] * 7 + [0]

    def bwd(P=0):
        a = _C.BackwardArgs()
        a.P, a.M, a.width, a.height, a.tan_fovx, a.tan_fovy = P, 1, 8, 8, 1.0, 1.0
        if P:   # pointers that pass the stage's own checks; none is dereferenced before the range check
            for n in ("background", "means3D", "viewmatrix", "projmatrix", "geometry", "image", "dL_dpix", "dL_dmean2D", "dL_dopacity",
                      "dL_dmean3D", "dL_dscale", "dL_drot", "scales", "rotations", "colors_precomp", "dL_dcolor"):
                setattr(a, n, aligned)
        return a

    # aux == NULL and an unknown mode, every *_aux entry point (P == 0: only the option's check can object)
    calls = ((L.gsr_forward_preprocess_aux, lambda x: [x] + pre()), (L.gsr_forward_preprocess_leaf_aux, lambda x: [x] + pre_leaf()),
             (L.gsr_forward_render_aux, lambda x: [x] + render()), (L.gsr_backward_blend_aux, lambda x: [ctypes.byref(bwd()), x]),
             (L.gsr_backward_gaussians_aux, lambda x: [ctypes.byref(bwd()), x, 0, 0, 0]))
    for fn, args in calls:
        assert fn(*args(None)) == BAD and err().startswith(fn.__name__.encode()), fn.__name__
        assert fn(*args(ctypes.byref(aux_args(mode=3)))) == BAD and err().startswith(fn.__name__.encode()), fn.__name__
        assert fn(*args(ctypes.byref(aux_args()))) == OK and err() == b"", fn.__name__    # P == 0: nothing is launched
    assert R.value == 0   # (what stage 1 reports for an empty scene)
    # the blend needs the outputs and the scratch, 16-byte aligned; the backward calls an aligned scratch
    assert L.gsr_forward_render_aux(ctypes.byref(aux_args(out=None)), *render(P=1)) == BAD and err().startswith(b"gsr_forward_render_aux")
    assert L.gsr_forward_render_aux(ctypes.byref(aux_args(scratch=aligned + 4)), *render()) == BAD and err().startswith(b"gsr_forward_render_aux")
    assert L.gsr_backward_blend_aux(ctypes.byref(bwd()), ctypes.byref(aux_args(scratch=aligned + 4))) == BAD
    assert err().startswith(b"gsr_backward_blend_aux")
    assert L.gsr_backward_gaussians_aux(ctypes.byref(bwd()), ctypes.byref(aux_args(scratch=aligned + 4)), 0, 0, 0) == BAD
    assert err().startswith(b"gsr_backward_gaussians_aux")
    # the filter's per-Gaussian backward: the opacity input, and the range's first Gaussian a multiple of 64
    assert L.gsr_backward_gaussians_aa(ctypes.byref(bwd(P=128)), 1, None, None, 0, 64, 0) == BAD and err().startswith(b"gsr_backward_gaussians_aa")
    assert L.gsr_backward_gaussians_aa(ctypes.byref(bwd(P=128)), 1, aligned, None, 32, 64, 0) == BAD and err().startswith(b"gsr_backward_gaussians")
    assert L.gsr_backward_gaussians_aa(ctypes.byref(bwd(P=128)), 1, aligned, None, 64, 0, 0) == OK     # an empty range: nothing is launched
    assert L.gsr_backward_gaussians_aa(ctypes.byref(bwd(P=128)), 0, None, None, 32, 64, 0) == BAD
    # with the option off the call is its default: the same verdict on the same invalid image size
    rc = L.gsr_forward_preprocess(*pre(P=1, width=0))
    assert rc == BAD and b"bad" in err()
    assert L.gsr_forward_preprocess_aa(0, None, *pre(P=1, width=0)) == rc and b"bad" in err()


def test_8f_python_surfaces_refuse_cpu_tensors():
    import fused_loss
    import fused_params
    from simple_knn._C import distCUDA2
    import diff_gaussian_rasterization as dgr
    with pytest.raises(RuntimeError, match="no CPU path"):
        distCUDA2(torch.zeros(8, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused_loss.l1_ssim_loss(torch.zeros(3, 8, 8), torch.zeros(3, 8, 8))
    p = torch.nn.Parameter(torch.zeros(4, 3))
    p.grad = torch.ones(4, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused_params.FusedAdam([{"params": [p], "lr": 1e-3, "name": "xyz"}], lr=0.0, eps=1e-15).step()
    s = dgr.GaussianRasterizationSettings(16, 16, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                          torch.zeros(3), False, False)
    m = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused_params.rasterize_leaf_gaussians(m, m, torch.zeros(4, 1, 3), torch.zeros(4, 0, 3), torch.zeros(4, 1), m, torch.zeros(4, 4), s)


def test_no_barrier_with_an_lds_access_in_flight():
    """`make audit`: the gfx950 ISA of every translation unit, checked by tools/barrier_audit.py -- no s_barrier may be reachable
    while one of the wave's LDS accesses can still be outstanding (hipcc 7.2 dropped the release fence's s_waitcnt on a loop back
    edge of the depth sort once; gsr_depth_key.h, gsr_sync()).  Cross-compiles here, needs no GPU."""
    import shutil
    import subprocess
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc / make")
    csrc = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "csrc")
    p = subprocess.run(["make", "-j8", "audit"], cwd=csrc, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert p.stdout.count("0 barriers reachable") >= 11, p.stdout[-3000:]


def test_barrier_audit_sees_a_missing_wait(tmp_path):
    """The checker itself, on two hand-written kernels: a store to LDS followed by a barrier with and without the wait, the
    second one through a loop back edge (the shape of the compiler's miss)."""
    import subprocess
    import sys
    good = tmp_path / "good.s"
    bad = tmp_path / "bad.s"
    body = "k:\n\tds_write_b32 v0, v1\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier\n\ts_endpgm\n"
    good.write_text(body)
    bad.write_text("k:\n.LBB0_1:\n\ts_barrier\n\tds_read_b32 v2, v0\n\ts_waitcnt lgkmcnt(0)\n\tds_write_b32 v0, v1\n\ts_cbranch_scc1 .LBB0_1\n\ts_endpgm\n")
    tool = os.path.join(ROOT, "tools", "barrier_audit.py")
    assert subprocess.run([sys.executable, tool, str(good)]).returncode == 0
    r = subprocess.run([sys.executable, tool, str(bad)], capture_output=True, text=True)
    assert r.returncode == 1 and "bad.s:3" in r.stdout


def test_trim_word_decoder_host_and_numpy_restatement_agree():
    """csrc/gsr_rect_trim.h's decoder (what pass 1 of the binning does with a rectangle's trim word) compiled for the host
    (tests/cpp/trim_decode.cpp) against tests/util.trim_kept -- the numpy restatement from which the GPU parity tests derive the lists
    they expect -- on random rectangles of every size class (one nibble per column / per group of 2 .. 32 columns, rows in units of
    1 .. 16) and random words, including words no producer writes (empty groups between kept ones)."""
    import shutil
    import subprocess
    import sys
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import util
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    exe = os.path.join(ROOT, "tests", "cpp", "trim_decode")
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "trim_decode.cpp")],
                   check=True, capture_output=True)
    r = np.random.default_rng(11)
    n = 4000
    w = r.choice([1, 2, 3, 5, 8, 9, 13, 16, 17, 31, 32, 33, 64, 100, 200, 256], n)
    h = r.choice([1, 2, 4, 6, 7, 15, 16, 17, 32, 33, 64, 129, 256], n)
    x0 = (r.random(n) * (257 - w)).astype(np.int64)
    y0 = (r.random(n) * (257 - h)).astype(np.int64)
    trim = r.integers(0, 1 << 32, n, dtype=np.uint64)
    trim[::5] = 0
    trim[1::7] = 0xFFFFFFFF
    packed = (x0 | (y0 << 8) | ((w - 1) << 16) | ((h - 1) << 24)).astype(np.uint64)
    out = subprocess.run([exe], input="".join(f"{int(p)} {int(t)}\n" for p, t in zip(packed, trim)), capture_output=True, text=True, check=True).stdout.split("\n")
    rshape = np.stack([packed, trim], 1).astype(np.uint32)
    gx = 256
    for k in range(n):
        tx, ty = np.meshgrid(np.arange(x0[k], x0[k] + w[k]), np.arange(y0[k], y0[k] + h[k]))
        tiles = (ty * gx + tx).reshape(-1)
        want = util.trim_kept(rshape, np.full(tiles.shape, k), tiles, gx)
        got = np.frombuffer(out[k].encode(), np.uint8) == ord("1")
        assert np.array_equal(got, want), (k, int(w[k]), int(h[k]), hex(int(trim[k])))


def _frame_entry_points():
    """The entry points that open the state of a forward, as rows of a table: name, a call taking (P, R, W, H, buffers), the
    buffers it takes, those it refuses as NULL, those it refuses misaligned, and whether it limits R to 32 bits."""
    from diff_gaussian_rasterization import _C
    L = _C.lib()
    BWD_REQUIRED = ("background", "means3D", "viewmatrix", "projmatrix", "geometry", "image", "dL_dpix", "dL_dmean2D", "dL_dopacity",
                    "dL_dmean3D", "dL_dscale", "dL_drot", "binning", "scratch")
    BWD_POINTERS = tuple(n for n, t in _C.BackwardArgs._fields_ if t is ctypes.c_void_p and n != "stream")

    def bwd(P, R, W, H, b):
        a = _C.BackwardArgs()
        a.P, a.num_rendered, a.width, a.height, a.M, a.tan_fovx, a.tan_fovy = P, R, W, H, 1, 1.0, 1.0
        for n in BWD_POINTERS:
            if n in b:
                setattr(a, n, b[n])
        return ctypes.byref(a)

    state = ("geometry", "binning", "image")
    aux = lambda: ctypes.byref(_C.AuxArgs(1, 4096, 4096, None, None, 4096))
    rows = []
    add = lambda name, call, buffers, required, aligned, limit, **kw: rows.append(dict(name=name, call=call, buffers=buffers, required=required,
                                                                                       aligned=aligned, limit=limit, **kw))
    render = lambda fn, *lead: lambda P, R, W, H, b: fn(*lead, P, R, W, H, b.get("background"), b.get("radii"), b.get("geometry"),
                                                        b.get("binning"), b.get("image"), b.get("out_color"), None, 0)
    add("gsr_forward_render", render(L.gsr_forward_render), state + ("background", "radii", "out_color"), state + ("background", "out_color"), state, True)
    add("gsr_forward_render_aux", lambda P, R, W, H, b: render(L.gsr_forward_render_aux, aux())(P, R, W, H, b),
        state + ("background", "radii", "out_color"), state + ("background", "out_color"), state, True)
    # (the blend with nothing rendered, and the per-Gaussian pass over an empty range, return before any launch)
    add("gsr_backward_blend", lambda P, R, W, H, b: L.gsr_backward_blend(bwd(P, R, W, H, b)), BWD_POINTERS, BWD_REQUIRED,
        state + ("scratch",), False, only_if_rendered=("binning", "scratch"))
    add("gsr_backward_blend_abs", lambda P, R, W, H, b: L.gsr_backward_blend_abs(bwd(P, R, W, H, b), None, 1), BWD_POINTERS, BWD_REQUIRED,
        state + ("scratch",), False, only_if_rendered=("binning", "scratch"))
    add("gsr_backward_gaussians", lambda P, R, W, H, b: L.gsr_backward_gaussians(bwd(P, R, W, H, b), 0, max(P, 0) if R else 0, 0), BWD_POINTERS,
        BWD_REQUIRED, state + ("scratch",), False, only_if_rendered=("binning", "scratch"))
    # (the fold reads no image; one of its two outputs must be there whatever P is)
    add("gsr_absgrad_fold", lambda P, R, W, H, b: L.gsr_absgrad_fold(bwd(P, R, W, H, b), ctypes.byref(_C.AbsgradArgs(b.get("abs_dL_dmean2D", 4096), None)),
                                                                    0, max(P, 0)),
        ("geometry", "binning", "scratch"), ("geometry", "binning", "scratch"), ("geometry", "binning", "scratch"), False)
    add("gsr_contributions", lambda P, R, W, H, b: L.gsr_contributions(P, R, W, H, b.get("geometry"), b.get("binning"), b.get("image"),
                                                                       b.get("pixel_weight"), b.get("weight_sum"), b.get("weight_max"),
                                                                       b.get("pixel_count"), b.get("own_scratch"), None, 0),
        state + ("pixel_weight", "weight_sum", "weight_max", "pixel_count", "own_scratch"), state + ("own_scratch",), state + ("own_scratch",), True,
        only_if_rendered=("binning", "own_scratch"))
    add("gsr_features_forward", lambda P, R, W, H, b: L.gsr_features_forward(P, R, W, H, 4, b.get("geometry"), b.get("binning"), b.get("image"),
                                                                             b.get("features"), b.get("out"), None, 0),
        state + ("features", "out"), state + ("features", "out"), state, True)
    add("gsr_features_backward", lambda P, R, W, H, b: L.gsr_features_backward(bwd(P, R, W, H, b), 4, b.get("features"), b.get("dL_dout"),
                                                                               b.get("dL_dfeatures"), b.get("own_scratch"), 1),
        state + ("scratch", "features", "dL_dout", "dL_dfeatures", "own_scratch"), state + ("scratch", "features", "dL_dout", "dL_dfeatures", "own_scratch"),
        state + ("scratch", "own_scratch"), True)
    add("gsr_distortion_forward", lambda P, R, W, H, b: L.gsr_distortion_forward(P, R, W, H, b.get("geometry"), b.get("binning"), b.get("image"),
                                                                                 b.get("out"), b.get("state"), None, 0),
        state + ("out", "state"), state + ("out", "state"), state + ("state",), True)
    add("gsr_distortion_backward", lambda P, R, W, H, b: L.gsr_distortion_backward(bwd(P, R, W, H, b), b.get("state"), b.get("dL_dmap")),
        state + ("scratch", "state", "dL_dmap"), state + ("scratch", "state", "dL_dmap"), state + ("scratch", "state"), True,
        only_if_rendered=("binning", "scratch"))
    add("gsr_median_forward", lambda P, R, W, H, b: L.gsr_median_forward(P, R, W, H, b.get("geometry"), b.get("binning"), b.get("image"),
                                                                         b.get("out"), b.get("out_index"), b.get("out_dominant"),
                                                                         b.get("out_weight"), b.get("state"), None, 0),
        state + ("out", "out_index", "out_dominant", "out_weight", "state"), state + ("state",), state + ("state",), True)
    add("gsr_median_backward", lambda P, R, W, H, b: L.gsr_median_backward(bwd(P, R, W, H, b), b.get("state"), b.get("dL_dmap")),
        state + ("scratch", "state", "dL_dmap"), state + ("scratch", "state", "dL_dmap"), state + ("scratch", "state"), True,
        only_if_rendered=("binning", "scratch"))
    return L, rows


def frame_refusal_table():
    """Every row of test_frame_entry_points_refuse_alike: (entry point, description of the fault, return code, message)."""
    L, rows = _frame_entry_points()
    one, odd = 4096, 4104   # never dereferenced: 16-byte aligned, and 8-byte aligned only
    out = []
    for e in rows:
        def run(what, P=4, R=8, W=32, H=16, **change):
            b = {n: one for n in e["buffers"]}
            b.update(change)
            rc = e["call"](P, R, W, H, b)
            out.append((e["name"], what, dict(P=P, R=R, W=W, H=H, **change), rc, L.gsr_last_error()))
        for kw in (dict(P=-1), dict(R=-1), dict(W=0), dict(H=-3)):
            run("sizes", **kw)
        for n in e["required"]:
            run("null", **{n: None})
        for n in e["aligned"]:
            run("align", **{n: odd})
        if e["limit"]:
            run("limit", R=1 << 32)
        first = e["aligned"][0]
        run("sizes before null", W=0, **{first: None})
        run("null before align", **{first: None, e["aligned"][1]: odd})
        if e["limit"]:
            run("align before limit", R=1 << 32, **{first: odd})
        if e.get("only_if_rendered"):
            run("nothing rendered", R=0, **{n: None for n in e["only_if_rendered"]})
        run("empty scene", P=0, **{n: None for n in e["buffers"]})
    return out


# the variants of one call report under that call's name
_FRAME_SAID_BY = {"gsr_forward_render_aux": "gsr_forward_render", "gsr_backward_blend_abs": "gsr_backward_blend"}


def test_frame_entry_points_refuse_alike():
    """Every entry point that opens the state of a forward (geometry, image, binning, gradient slots), with P=4, R=8, a 32 x 16 image
    and fake addresses that are never dereferenced, and exactly one fault at a time: bad sizes, each required buffer NULL, each buffer
    whose alignment matters 8-byte aligned only, and R = 2^32 where the entry point limits R (the backward calls do not).  Each is
    GSR_ERR_INVALID_ARGUMENT with a message under the entry point's name.  Of two faults the earlier class is reported: sizes, NULL,
    alignment, the limit on R.  binning and the slots are needed only when something was rendered, and an empty scene is GSR_OK with
    every pointer NULL and an empty gsr_last_error().  A valid call would launch, so none is made: nothing here touches a device."""
    table = frame_refusal_table()
    assert len({r[0] for r in table}) >= 12
    single = {}
    for name, what, args, rc, msg in table:
        key = (name, what, tuple(sorted((k, v) for k, v in args.items() if (k, v) not in (("P", 4), ("R", 8), ("W", 32), ("H", 16)))))
        single[key] = msg
        if what in ("sizes", "null", "align", "limit"):
            assert rc == -1 and msg, (name, args, rc, msg)
            said_by = _FRAME_SAID_BY.get(name, name)
            assert msg.decode().startswith(said_by + ":"), (name, args, msg)
            if what == "sizes":
                assert b"bad" in msg, (name, args, msg)
        elif what in ("nothing rendered", "empty scene"):
            assert rc == 0 and msg == b"", (name, what, args, rc, msg)
    # of two faults the earlier class is reported: the pair's message is the earlier fault's own
    for name, what, args, rc, msg in table:
        if " before " not in what:
            continue
        assert rc == -1, (name, what, args, rc)
        extra = {k: v for k, v in args.items() if (k, v) not in (("P", 4), ("R", 8), ("W", 32), ("H", 16))}
        if what == "sizes before null":
            earlier = {"W": 0}
        elif what == "null before align":
            earlier = {k: v for k, v in extra.items() if v is None}
        else:
            earlier = {k: v for k, v in extra.items() if k != "R"}
        cls = what.split(" ")[0]
        assert msg == single[(name, cls, tuple(sorted(earlier.items())))], (name, what, args, msg)
