"""GPU: the per-Gaussian pass (csrc/gaussian_backward.hip, gaussian_backward_tail.inc) and its forward twin, the colour kernel of
csrc/preprocess.hip, where they can be wrong with the rest of the suite green.  The scenes have at most 333 Gaussians on 128 x 96
pixels: the kernels' edge cases are the whole workload.

A  The leaf-activation backward (exp, sigmoid, F.normalize folded into the kernel) against tests/torch_leaf.py in float64, per
   Gaussian, on leaves with saturated logits, log-scales from -9 to 1 and quaternion norms from 1e-3 to 1e3 (fixture A, whose
   conditions tests/test_leaf_reference_cpu.py asserts).  g_act is what the non-leaf backward returns for the torch-activated values
   of the same leaves.  For each leaf, max err_kernel <= 2 max err_stock + 2^-22: err the normalised error of torch_leaf (c),
   stock the fp32 chain PyTorch runs (torch_leaf (b)) on the device the kernel ran on, so both see the same activated bits; the
   factor 2 is for another operation order and the floor for a one-ulp difference of an expf; neither is a measured figure.  Held
   over all visible rows and over those with |logit| <= 8, so that the saturated band, where stock itself loses the digits of
   1 - y, cannot lend its slack to the rest.
B  gsr_backward_gaussians part by part -- a part that is one wave, one that is a single Gaussian at an odd multiple of 64, one
   that ends in mid-wave, one that ends the scene in mid-wave -- into outputs prefilled with 0xFF bytes, with out_row0 = 0 (whole-
   scene tensors) and out_row0 = first (a buffer of the part's rows): the part's rows have the bits of a whole-scene run, every
   other row and 64 guard rows behind the last keep the canary, the statistics change on the part's visible Gaussians alone.
C  M = 16 with an SH tensor that is 4-byte but not 16-byte aligned, the input or the gradient, packed and leaf: the kernels must
   take their per-lane path (the LDS block path moves float4), which no aligned torch allocation ever selects."""
import types

import numpy as np
import pytest
import torch

import gsr_scene
import torch_leaf as tl
import util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
W, H = 128, 96
BG = torch.tensor([0.1, 0.2, 0.3])
LEAVES = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
_cache = {}


def _camera():
    return gsr_scene.make_camera(W, H)


def _settings(D):
    return util.hip_settings(types.SimpleNamespace(bg=BG), _camera(), D, DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _leaves_a(M):
    lv = tl.fixture_a()
    lv[2] = lv[2][:, :M - 1].contiguous()
    return [t.to(DEV) for t in lv]


# ---- A: leaf activations ------------------------------------------------------------------------------------------------------
def _leaf_run(M, D, aa):
    from fused_params import rasterize_leaf_gaussians
    lv = [t.clone().requires_grad_(True) for t in _leaves_a(M)]
    m2 = torch.zeros_like(lv[0], requires_grad=True)
    color, radii = rasterize_leaf_gaussians(lv[0], m2, lv[1], lv[2], lv[3], lv[4], lv[5], _settings(D), antialiasing=aa)
    color.backward(tl.upstream(W, H).to(DEV))
    grads = {n: (torch.zeros_like(t) if t.grad is None else t.grad) for n, t in zip(LEAVES, lv)}
    return color.detach(), radii, grads, m2.grad


def _case_a(M, D, aa):
    """-> the leaf run and the non-leaf run on the torch-activated values of the same leaves; computed once, never written to"""
    key = ("A", M, D, aa)
    if key not in _cache:
        from diff_gaussian_rasterization import GaussianRasterizer
        leaf = _leaf_run(M, D, aa)
        act = {k: v.detach().clone().requires_grad_(True) for k, v in tl.activated(_leaves_a(M)).items()}
        m2 = torch.zeros_like(act["means3D"], requires_grad=True)
        color, radii = GaussianRasterizer(_settings(D), antialiasing=aa)(means2D=m2, **act)
        color.backward(tl.upstream(W, H).to(DEV))
        torch.cuda.synchronize()
        _cache[key] = leaf, (color.detach(), radii, {k: v.grad for k, v in act.items()}, m2.grad)
    return _cache[key]


def _check_leaf_activations(M, D, aa):
    (color, radii, got, m2), (color0, radii0, g0, m20) = _case_a(M, D, aa)
    xyz, dc, fr, opacity, scaling, rotation = _leaves_a(M)
    P = xyz.shape[0]
    # the forward is the same, bit for bit, and so is everything no activation lies in front of
    assert torch.equal(radii, radii0) and torch.equal(color, color0)
    assert torch.equal(_bits(got["xyz"]), _bits(g0["means3D"])) and torch.equal(_bits(m2), _bits(m20))
    assert torch.equal(_bits(got["features_dc"]), _bits(g0["shs"][:, :1]))
    if M > 1:
        assert torch.equal(_bits(got["features_rest"]), _bits(g0["shs"][:, 1:]))
    else:
        assert got["features_rest"].numel() == 0

    g_act = (g0["opacities"], g0["scales"], g0["rotations"])
    raw = (opacity, scaling, rotation)
    ref = tl.reference(*raw, *g_act)
    stock = tl.stock(*raw, *g_act)
    kernel = {k: got[k] for k in ("opacity", "scaling", "rotation")}
    assert all(bool(torch.isfinite(v).all()) for v in kernel.values())
    e_kernel = tl.normalised_error(kernel, ref, *raw, *g_act)
    e_stock = tl.normalised_error(stock, ref, *raw, *g_act)
    vis = radii > 0
    assert int(vis.sum()) >= 0.6 * P and bool(vis[P - 1])
    inner = vis & (opacity[:, 0].abs() <= 8)
    failed = []
    for name, g in zip(("opacity", "scaling", "rotation"), g_act):
        live = vis & (g != 0).any(dim=1)
        for label, sel in (("visible", vis), ("|logit| <= 8", inner if name == "opacity" else vis)):
            achieved, st = float(e_kernel[name][sel].max()), float(e_stock[name][sel].max())
            print(f"M = {M}, aa = {aa}, {name}, {label} ({int(sel.sum())} Gaussians, {int((live & sel).sum())} with a gradient): "
                  f"stock fp32 {st:.3e}, kernel {achieved:.3e}, bar {2 * st + tl.FLOOR:.3e}")
            if not achieved <= 2 * st + tl.FLOOR:
                failed.append((name, label, achieved, st))
    assert not failed, failed
    # a gradient reaches every band of logits (tests/test_leaf_reference_cpu.py asserts it through the oracle)
    for lo, hi in tl.BANDS:
        band = vis & (opacity[:, 0].abs() >= lo) & (opacity[:, 0].abs() <= hi) & (g_act[0][:, 0] != 0)
        assert int(band.sum()) >= 10, (lo, hi, int(band.sum()))
    # logits of +-20: fp32 sigmoid is 1 (or 1 - y times y underflows): stock's bits, or zero
    assert float(g_act[0][tl.ROW_LOGIT_PLUS20, 0]) != 0
    for row in (tl.ROW_LOGIT_PLUS20, tl.ROW_LOGIT_MINUS20):
        v = kernel["opacity"][row]
        assert bool(torch.isfinite(v).all()) and (torch.equal(_bits(v), _bits(stock["opacity"][row])) or float(v) == 0.0), (row, float(v))
    # the zero quaternion: g / 1e-12 and nothing from q (every term of the covariance's dL/dq carries a component of q, so g_act
    # itself is zero on this row and so must the result be; the scale gradient of the same row is not)
    v, g = kernel["rotation"][tl.ROW_ZERO_QUAT].double(), g_act[2][tl.ROW_ZERO_QUAT].double()
    assert bool(torch.isfinite(v).all()) and bool(((v - g / 1e-12).abs() <= 1e-6 * (g / 1e-12).abs()).all())
    assert float(g_act[1][tl.ROW_ZERO_QUAT].abs().max()) > 0 and float(kernel["scaling"][tl.ROW_ZERO_QUAT].abs().max()) > 0


@pytest.mark.parametrize("antialiasing", (False, True))
def test_leaf_activation_backward_against_float64(antialiasing):
    """A1.  Measured on an MI355X: the kernel's figure equals stock's for every leaf and set."""
    _check_leaf_activations(16, 3, antialiasing)


@pytest.mark.parametrize("M,D", ((9, 2), (1, 0)))
def test_leaf_activation_backward_on_the_generic_sh_paths(M, D):
    """A2: per-lane SH rows (M = 9) and no rest tensor at all (M = 1)"""
    _check_leaf_activations(M, D, False)


def test_leaf_gradients_of_culled_rows_are_plus_zero_and_runs_repeat():
    """A3"""
    (color, radii, got, m2), _ = _case_a(16, 3, False)
    culled = radii <= 0
    assert int(culled.sum()) >= 20
    for name in LEAVES:
        assert bool((_bits(got[name])[culled] == 0).all()), name   # +0: no bit set
    assert bool((_bits(m2)[culled] == 0).all())
    color2, radii2, got2, m22 = _leaf_run(16, 3, False)
    assert torch.equal(color, color2) and torch.equal(radii, radii2) and torch.equal(_bits(m2), _bits(m22))
    for name in LEAVES:
        assert torch.equal(_bits(got[name]), _bits(got2[name])), name


# ---- the two-stage backward, by hand --------------------------------------------------------------------------------------------
def _forward(layout, lv, D, M):
    """-> (R, color, radii, geom, binning, img, inputs of the backward)"""
    from diff_gaussian_rasterization import _C
    import fused_params
    st = _settings(D)
    if layout == "leaf":
        R, color, radii, geom, binning, img, M_, kept = fused_params.leaf_forward(lv[0], lv[1], lv[2], lv[3], lv[4], lv[5], st)
        assert M_ == M
        return R, color, radii, geom, binning, img, kept
    e = torch.empty(0, device=DEV)
    R, color, radii, geom, binning, img = _C.rasterize_gaussians(
        st.bg, lv["means3D"], e, lv["opacities"], lv["scales"], lv["rotations"], 1.0, e, st.viewmatrix, st.projmatrix, st.tanfovx,
        st.tanfovy, H, W, lv["shs"], D, st.campos, False, False)
    return R, color, radii, geom, binning, img, lv


def _backward_args(layout, fwd, D, M, dpix):
    """-> (BackwardArgs after the blend pass, the tensors it points to)"""
    from diff_gaussian_rasterization import _C
    import fused_params
    st = _settings(D)
    R, color, radii, geom, binning, img, inp = fwd
    P = radii.shape[0]
    scratch = _C.backward_scratch(P, R, DEV)
    if layout == "leaf":
        xyz, fdc, frest, scaling, rotation = inp
        a = fused_params.leaf_backward_args(st, R, M, xyz, fdc, frest, scaling, rotation, radii, geom, binning, img, scratch, dpix)
    else:
        a = _C.backward_args(P=P, D=D, M=M, R=R, W=W, H=H, leaf=0, background=st.bg, means3D=inp["means3D"], shs=inp["shs"],
                             scales=inp["scales"], scale_modifier=1.0, rotations=inp["rotations"], viewmatrix=st.viewmatrix,
                             projmatrix=st.projmatrix, cam_pos=st.campos, tan_fovx=st.tanfovx, tan_fovy=st.tanfovy, radii=radii,
                             geometry=geom, binning=binning, image=img, scratch=scratch, dL_dpix=dpix, debug=False, device=DEV)
    return a, (st, scratch, dpix, fwd)


def _widths(layout, M, sh=True):
    w = dict(dL_dmean2D=3, dL_dmean3D=3, dL_dopacity=1, dL_dscale=3, dL_drot=4, dL_dcolor=3, dL_dconic=4, dL_dcov3D=6)
    if sh and layout == "leaf":
        w.update(dL_dsh=3, dL_dsh_rest=3 * (M - 1))
    elif sh:
        w.update(dL_dsh=3 * M)
    return w


GUARD = 64


def _canary_outputs(widths, rows):
    """rows + GUARD rows of 0xFF bytes per output (NaNs as floats), as int32"""
    return {k: torch.full(((rows + GUARD) * w,), -1, dtype=torch.int32, device=DEV).view(rows + GUARD, w) for k, w in widths.items()}


STATS0 = (1.5, 3.0, 0.25)   # xyz_gradient_accum, denom, max_radii2D before a pass


def _stats(P):
    return tuple(torch.full((P,), v, dtype=torch.float32, device=DEV) for v in STATS0)


def _case_b(layout, M, skip_dsh=False):
    """One forward, one blend pass and the whole-scene per-Gaussian pass of fixture B: the expectation of every part"""
    key = ("B", layout, M, skip_dsh)
    if key not in _cache:
        from diff_gaussian_rasterization import _C
        D = {16: 3, 9: 2}[M]
        lv = tl.fixture_b()
        lv[2] = lv[2][:, :M - 1].contiguous()
        lv = [t.to(DEV) for t in lv]
        fwd = _forward(layout, lv if layout == "leaf" else tl.activated(lv), D, M)
        P = lv[0].shape[0]
        a, keep = _backward_args(layout, fwd, D, M, tl.upstream(W, H).to(DEV))
        widths = _widths(layout, M, sh=not skip_dsh)
        whole, stats = _canary_outputs(widths, P), _stats(P)
        _C.set_backward_outputs(a, dL_dsh=None, dL_dsh_rest=None)
        _C.set_backward_outputs(a, **whole)
        _C.set_backward_stats(a, stats, P, DEV)
        _C.backward_blend(a)
        _C.backward_gaussians(a, 0, P, 0)
        torch.cuda.synchronize()
        for k, t in whole.items():
            assert bool((t[P:] == -1).all()), k
            assert bool(torch.isfinite(t[:P].view(torch.float32)).all()), k
        _cache[key] = a, keep, widths, whole, stats, fwd[2], lv
    return _cache[key]


def _run_parts(layout, M, out_row0_is_first, skip_dsh=False):
    """Every part of fixture B into canary-filled outputs -> {(first, count): the part's rows per output}"""
    from diff_gaussian_rasterization import _C
    a, keep, widths, whole, stats_whole, radii, lv = _case_b(layout, M, skip_dsh)
    P = radii.shape[0]
    vis = radii > 0
    got = {}
    for first, count in tl.PARTS_B:
        rows = count if out_row0_is_first else P
        out, stats = _canary_outputs(widths, rows), _stats(P)
        _C.set_backward_outputs(a, **out)
        _C.set_backward_stats(a, stats, P, DEV)
        _C.backward_gaussians(a, first, count, first if out_row0_is_first else 0)
        torch.cuda.synchronize()
        lo = 0 if out_row0_is_first else first
        inside = torch.zeros(rows + GUARD, dtype=torch.bool, device=DEV)
        inside[lo:lo + count] = True
        for k, t in out.items():
            # the part's rows: the bits of the whole-scene run; every other row and the guard rows: the canary's bytes
            assert torch.equal(t[inside], whole[k][first:first + count]), (k, first, count)
            assert bool((t[~inside] == -1).all()), (k, first, count, "rows outside the part were written")
        in_part = torch.zeros(P, dtype=torch.bool, device=DEV)
        in_part[first:first + count] = True
        touched = in_part & vis
        assert int(touched.sum()) >= 1
        for k, (s, sw, v0) in enumerate(zip(stats, stats_whole, STATS0)):
            assert torch.equal(s[in_part], sw[in_part]), (k, first, count)
            assert bool((s[~touched] == v0).all()), (k, first, count, "a statistic changed outside the part's visible Gaussians")
        assert bool((stats[1][touched] == STATS0[1] + 1).all())
        assert torch.equal(stats[2][touched], radii[touched].float()) and bool((radii[touched] >= 1).all())
        got[(first, count)] = {k: t[inside] for k, t in out.items()}
    return got


@pytest.mark.parametrize("out_row0", ("0", "first"))
@pytest.mark.parametrize("M", (16, 9))
@pytest.mark.parametrize("layout", ("packed", "leaf"))
def test_backward_gaussians_part_by_part(layout, M, out_row0):
    """B1"""
    _run_parts(layout, M, out_row0 == "first")
    a, keep, widths, whole, stats, radii, lv = _case_b(layout, M)
    P = radii.shape[0]
    culled = radii <= 0
    # what the whole-scene run is: zeros on culled rows, something on the others
    for k in widths:
        assert bool((whole[k][:P][culled] == 0).all()), k
    assert bool((whole["dL_dsh"][:P][~culled] != 0).any(dim=1).float().mean() > 0.5)


@pytest.mark.parametrize("out_row0", ("0", "first"))
def test_backward_gaussians_part_by_part_in_view_parallel_mode(out_row0):
    """B2: no dL_dsh, dL_dcolor carries the clamp-masked dL/dRGB; gsr_sh_grad_from_views of the assembled parts gives the
    whole-scene dL_dsh"""
    from diff_gaussian_rasterization import _C
    got = _run_parts("packed", 16, out_row0 == "first", skip_dsh=True)
    a, keep, widths, whole, stats, radii, lv = _case_b("packed", 16, skip_dsh=True)
    full = _case_b("packed", 16)[3]
    P = radii.shape[0]
    for k in widths:   # nothing but dL_dcolor differs from the run with dL_dsh
        if k != "dL_dcolor":
            assert torch.equal(whole[k], full[k]), k
    rgb = torch.zeros(P, 3, dtype=torch.float32, device=DEV)
    covered = torch.zeros(P, dtype=torch.bool, device=DEV)
    for (first, count), out in got.items():
        rgb[first:first + count] = out["dL_dcolor"].view(torch.float32)
        covered[first:first + count] = True
    st = keep[0]
    dsh = _C.sh_grad_from_views(lv[0], st.campos[None], rgb[None], 3, 16)
    want = full["dL_dsh"][:P].view(torch.float32).view(P, 16, 3)
    # equal as numbers, as everywhere the two are compared: the fold adds its views to +0, so where the per-Gaussian pass stores the
    # product of a negative basis value and a clamped channel's 0, a -0, the fold returns +0
    differ = dsh[covered] != want[covered]
    assert not bool(differ.any()), (int(differ.sum()), float((dsh[covered] - want[covered]).abs().max()))
    odd = _bits(dsh[covered]) != _bits(want[covered])
    print(f"view-parallel parts: {int(odd.sum())} of {odd.numel()} elements differ in the sign of a zero, none in value")
    assert bool((want[covered][odd] == 0).all())
    assert bool((_bits(dsh[~covered]) == 0).all()) and float(want[covered].abs().max()) > 0


# ---- C: SH tensors that are not 16-byte aligned ---------------------------------------------------------------------------------
def _displaced(t, k):
    """a contiguous copy of t that starts k floats into a larger allocation"""
    big = torch.zeros(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = big[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * k and v.data_ptr() % 16 != 0
    return v


def _run_c(layout, displace=None, k=1):
    """Fixture A through the two-stage backward with every output given; displace: the tensor that starts k floats off
    -> dict(state, grads (float32 tensors), canaries (int32 tensors that must still hold -1))"""
    from diff_gaussian_rasterization import _C
    M, D = 16, 3
    lv = _leaves_a(M)
    P = lv[0].shape[0]
    if layout == "leaf":
        if displace == "features_rest":
            lv[2] = _displaced(lv[2], k)
        if displace == "features_dc":
            lv[1] = _displaced(lv[1], k)
        inp = lv
    else:
        inp = dict(_case_c_inputs())
        if displace == "shs":
            inp["shs"] = _displaced(inp["shs"], k)
    fwd = _forward(layout, inp, D, M)
    a, keep = _backward_args(layout, fwd, D, M, _case_c_dpix().to(DEV))
    widths = _widths(layout, M)
    bufs, outs = {}, {}
    for name, w in widths.items():
        off = k if name == displace else 0
        bufs[name] = torch.full((off + P * w + GUARD,), -1, dtype=torch.int32, device=DEV)
        outs[name] = bufs[name][off:off + P * w]
        if off:
            assert outs[name].data_ptr() % 16 != 0
    _C.set_backward_outputs(a, **outs)
    _C.backward_blend(a)
    _C.backward_gaussians(a, 0, P, 0)
    torch.cuda.synchronize()
    R, color, radii, geom, binning, img = fwd[:6]
    state = util.unpack_state(dict(R=R, geom=geom, binning=binning, img=img), P, W, H)
    gl = _C.geometry_layout(P)
    state["sh_ddir"] = geom[gl.sh_ddir:gl.sh_ddir + 36 * P].cpu().numpy().view(np.float32).reshape(9, P)
    state.update(color=color.cpu().numpy(), radii=radii.cpu().numpy(), num_rendered=R)
    grads = {name: outs[name].view(torch.float32).view(P, -1).cpu().numpy() for name in widths}
    canaries = {name: (bufs[name][:k if name == displace else 0], bufs[name][-GUARD:]) for name in widths}
    return dict(state=state, grads=grads, canaries=canaries)


def _case_c_inputs():
    """fixture A's activated values, by torch on the device (what the oracle is fed with, copied to the host)"""
    if "C_inputs" not in _cache:
        _cache["C_inputs"] = {k: v.contiguous() for k, v in tl.activated(_leaves_a(16)).items()}
    return _cache["C_inputs"]


def _case_c_oracle():
    if "C_oracle" not in _cache:
        act = {k: v.cpu() for k, v in _case_c_inputs().items()}
        scene = gsr_scene.Scene(act["means3D"], act["scales"], act["rotations"], act["opacities"], act["shs"], BG)
        o = util.oracle_forward(scene, _camera(), 3)
        dpix = util.fragile_free_dpix(o, _camera())
        _cache["C_oracle"] = o, dpix, util.oracle.backward(o, dpix.numpy())
    return _cache["C_oracle"]


def _case_c_dpix():
    return _case_c_oracle()[1]


def _case_c_aligned(layout):
    if ("C", layout) not in _cache:
        _cache[("C", layout)] = _run_c(layout)
    return _cache[("C", layout)]


def _oracle_view(r):
    """the dict util.hip_forward_backward returns, of a _run_c result (packed layout)"""
    g = r["grads"]
    raw = dict(dL_dmeans2D=g["dL_dmean2D"], dL_dconic=g["dL_dconic"], dL_dopacity=g["dL_dopacity"], dL_dcolors=g["dL_dcolor"],
               dL_dmeans3D=g["dL_dmean3D"], dL_dcov3D=g["dL_dcov3D"], dL_dsh=g["dL_dsh"].reshape(-1, 16, 3), dL_dscales=g["dL_dscale"],
               dL_drotations=g["dL_drot"])
    return dict(r["state"], raw_grads=raw, grads=raw)


def test_fixture_a_aligned_packed_run_matches_the_oracle():
    """the aligned run C compares with is itself the oracle's, at the bars of tests/test_parity_gpu.py"""
    from test_parity_gpu import check_forward, check_grads
    o, dpix, og = _case_c_oracle()
    h = _oracle_view(_case_c_aligned("packed"))
    check_forward(h, o, _camera())
    check_grads(h, o, dpix, ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"], label="fixture A", og=og)


C_CASES = [("packed", "shs", 1), ("packed", "shs", 2), ("packed", "shs", 3), ("packed", "dL_dsh", 1),
           ("leaf", "features_rest", 1), ("leaf", "dL_dsh_rest", 1), ("leaf", "features_dc", 1)]


@pytest.mark.parametrize("layout,displace,k", C_CASES)
def test_unaligned_sh_tensors_take_the_per_lane_path(layout, displace, k):
    """C1.  Measured on an MI355X: rgb, clamp bits, the sh_ddir planes and every gradient have the bits of the aligned run."""
    from test_parity_gpu import check_forward, check_grads
    ref = _case_c_aligned(layout)
    r = _run_c(layout, displace, k)
    vis = ref["state"]["radii"] > 0
    assert np.array_equal(r["state"]["radii"], ref["state"]["radii"]) and vis.sum() > 150
    # forward: both paths evaluate gsr_sh_channel in the same order, and the file is built without contraction
    assert np.array_equal(r["state"]["rgb"][vis].view(np.int32), ref["state"]["rgb"][vis].view(np.int32))
    assert np.array_equal(r["state"]["clamped_bits"][vis], ref["state"]["clamped_bits"][vis])
    assert ref["state"]["clamped_bits"][vis].any() and (ref["state"]["rgb"][vis] > 0).any()
    # the chain-level bar of test_parity_gpu.check_grads, against the aligned run
    report = []
    a, b = r["state"]["sh_ddir"][:, vis], ref["state"]["sh_ddir"][:, vis]
    report.append(("sh_ddir", float(np.abs(a - b).max()), 1e-6 * float(np.abs(b).max()), np.array_equal(a.view(np.int32), b.view(np.int32))))
    for name, b in ref["grads"].items():
        a = r["grads"][name]
        assert float(np.abs(b).max()) > 0, name
        report.append((name, float(np.abs(a - b).max()), 1e-6 * float(np.abs(b).max()), np.array_equal(a.view(np.int32), b.view(np.int32))))
    for name, err, bar, same in report:
        print(f"{layout}, {displace} + {k}: {name:12s} max |unaligned - aligned| {err:.3e}, bar {bar:.3e}, same bits: {same}")
    assert all(err <= bar for _, err, bar, _ in report), report
    # nothing in front of or behind a displaced output was written
    for name, (front, behind) in r["canaries"].items():
        assert bool((front == -1).all()) and bool((behind == -1).all()), name
    if layout == "packed":
        o, dpix, og = _case_c_oracle()
        h = _oracle_view(r)
        check_forward(h, o, _camera())
        check_grads(h, o, dpix, ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"],
                    label=f"fixture A, {displace} + {k}", og=og)
