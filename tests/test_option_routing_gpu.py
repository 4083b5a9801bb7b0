"""GPU: the routing of the autograd layer -- which outputs a set of options returns and in which order, that an output outside the
loss changes no gradient, and which camera inputs receive a gradient -- through GaussianRasterizer ("plain") and
fused_params.rasterize_leaf_gaussians ("leaf") on the scene of the camera-gradient tests (P = 200, 40 x 24, six tiles).  Nothing here
has a tolerance: every comparison is torch.equal against another run of the same kernels on the same state, which the docstrings of
GaussianRasterizer promise ("colour, radii and maps have the same bits", "no gradient reached the map: nothing of it runs")."""
import pytest
import torch

import __graft_entry__  # noqa: F401
import torch_splat_cam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 5
MAPS = ("depth", "alpha", "distortion", "median_depth")
CAMERA_TARGET_HELPERS = ("camera_target",)   # the attributes of _C that allocate the camera gradients' struct and outputs
# option sets of the output-tuple test: the keywords and the maps they put behind (color, radii)
OPTION_SETS = {
    "none": ({}, ()),
    "depth": (dict(depth_alpha="depth"), ("depth", "alpha")),
    "depth_distortion": (dict(depth_alpha="depth", distortion=True), ("depth", "alpha", "distortion")),
    "depth_median": (dict(depth_alpha="depth", median_depth=True), ("depth", "alpha", "median_depth")),
    "depth_distortion_median": (dict(depth_alpha="depth", distortion=True, median_depth=True), MAPS),
}
# the smallest option set that has an output, and whether it needs `features`
SMALLEST = {"color": ("none", False), "depth": ("depth", False), "alpha": ("depth", False), "distortion": ("depth_distortion", False),
            "median_depth": ("depth_median", False), "feature_map": ("none", True)}
_CACHE = {}


def _scene():
    if "scene" not in _CACHE:
        scene, cam = torch_splat_cam.camera_test_scene()
        g = torch.Generator().manual_seed(17)
        H, W = cam.image_height, cam.image_width
        up = {n: torch.randn(1, H, W, generator=g).to(DEV) for n in MAPS}
        up["color"], up["feature_map"] = torch.randn(3, H, W, generator=g).to(DEV), torch.randn(K, H, W, generator=g).to(DEV)
        _CACHE["scene"] = scene, cam, torch.randn(scene.means3D.shape[0], K, generator=g), up
    return _CACHE["scene"]


def _settings(scene, cam, **replace):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    st = GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=scene.bg.to(DEV),
        scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(DEV), projmatrix=cam.full_proj_transform.to(DEV), sh_degree=3,
        campos=cam.camera_center.to(DEV), prefiltered=False, debug=False)
    return st._replace(**replace)


def render(kind, opts, features=False, settings=None, gaussians_require_grad=True):
    """One forward -> (outputs, the inputs by name: the Gaussians' and `features`)"""
    import gsr_model
    from diff_gaussian_rasterization import GaussianRasterizer
    from fused_params import rasterize_leaf_gaussians
    scene, cam, feats, _ = _scene()
    st = settings if settings is not None else _settings(scene, cam)
    rg = gaussians_require_grad
    f = feats.to(DEV).requires_grad_(True) if features else None
    if kind == "plain":
        t = {k: getattr(scene, k).to(DEV).clone().requires_grad_(rg) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
        t["means2D"] = torch.zeros_like(t["means3D"], requires_grad=rg)
        outs = GaussianRasterizer(st, **opts)(**t, features=f)
    else:
        pc = gsr_model.GaussianParams.from_activated(scene.means3D, scene.shs, scene.scales, scene.rotations, scene.opacities,
                                                     device=DEV, requires_grad=rg)
        t = dict(zip(("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity"), pc.parameters()),
                 means2D=torch.zeros_like(pc._xyz, requires_grad=rg))
        outs = rasterize_leaf_gaussians(pc._xyz, t["means2D"], pc._features_dc, pc._features_rest, pc._opacity, pc._scaling,
                                        pc._rotation, st, features=f, **opts)
    if f is not None:
        t["features"] = f
    return outs, t


def named(outs, maps, features):
    names = ("color", "radii") + tuple(maps) + (("feature_map",) if features else ())
    assert len(outs) == len(names), f"{len(outs)} outputs, expected {names}"
    return dict(zip(names, outs))


def reference_outputs(kind):
    """every output once, from the smallest option set that has it; computed once and left unchanged"""
    key = ("outputs", kind)
    if key not in _CACHE:
        ref = {}
        for name, (small, features) in SMALLEST.items():
            opts, maps = OPTION_SETS[small]
            with torch.no_grad():
                ref[name] = named(render(kind, opts, features)[0], maps, features)[name].clone()
        with torch.no_grad():
            ref["radii"] = render(kind, {})[0][1].clone()
        # a blank image would make every check of this file vacuous
        assert int((ref["radii"] > 0).sum()) > 50 and float((ref["alpha"] > 0.5).float().mean()) > 0.3, "the scene renders too little"
        for a in MAPS + ("feature_map",):
            assert float(ref[a].abs().max()) > 0, f"{a} is blank"
            for b in MAPS + ("feature_map",):
                assert a == b or ref[a].shape != ref[b].shape or not torch.equal(ref[a], ref[b]), f"{a} and {b} cannot be told apart"
        _CACHE[key] = ref
    return _CACHE[key]


@pytest.mark.parametrize("features", [False, True], ids=["nofeatures", "features"])
@pytest.mark.parametrize("option_set", list(OPTION_SETS))
@pytest.mark.parametrize("kind", ["plain", "leaf"])
def test_output_tuple(kind, option_set, features):
    """(color, radii[, depth, alpha][, distortion][, median_depth][, feature_map]): the documented order and shapes, and each output
    has the bits of the same output of the smallest option set that has it -- which an output in the wrong place would not."""
    scene, cam, _, _ = _scene()
    P, H, W = scene.means3D.shape[0], cam.image_height, cam.image_width
    ref = reference_outputs(kind)
    opts, maps = OPTION_SETS[option_set]
    res = named(render(kind, opts, features)[0], maps, features)
    shapes = dict(color=(3, H, W), radii=(P,), feature_map=(K, H, W), **{m: (1, H, W) for m in MAPS})
    for name, t in res.items():
        assert tuple(t.shape) == shapes[name], (name, tuple(t.shape))
        assert t.dtype == (torch.int32 if name == "radii" else torch.float32), (name, t.dtype)
        assert torch.equal(t, ref[name]), f"{name} differs from the {SMALLEST.get(name, ('none',))[0]} render's"
        assert t.requires_grad == (name != "radii"), name


@pytest.mark.parametrize("kind", ["plain", "leaf"])
def test_index_maps_alone(kind):
    """index_maps without any other option: the tuple stays (color, radii) and the three tensors are written in place"""
    scene, cam, _, _ = _scene()
    H, W = cam.image_height, cam.image_width
    ref = reference_outputs(kind)
    maps = (torch.full((H, W), -7, dtype=torch.int32, device=DEV), torch.full((1, H, W), -7, dtype=torch.int32, device=DEV),
            torch.full((H, W), -7.0, device=DEV))
    res = named(render(kind, dict(index_maps=maps))[0], (), False)
    assert torch.equal(res["color"], ref["color"]) and torch.equal(res["radii"], ref["radii"])
    blended = ref["alpha"].reshape(H, W) > 0
    for t in maps[:2]:
        assert bool(((t.reshape(H, W) >= 0) == blended).all()) and int(t.min()) >= -1 and int(t.max()) < scene.means3D.shape[0]
    assert bool(((maps[2] > 0) == blended).all())


@pytest.mark.parametrize("output", list(SMALLEST))
@pytest.mark.parametrize("kind", ["plain", "leaf"])
def test_unused_outputs_change_nothing(kind, output):
    """The loss on exactly one output: every input gradient from the largest option set (depth, distortion, median_depth and
    features) is torch.equal to the one from the smallest set that has the output."""
    _, _, _, up = _scene()
    reference_outputs(kind)
    grads = {}
    for which, (set_name, features) in (("small", SMALLEST[output]), ("large", ("depth_distortion_median", True))):
        opts, maps = OPTION_SETS[set_name]
        outs, inputs = render(kind, opts, features)
        (named(outs, maps, features)[output] * up[output]).sum().backward()
        torch.cuda.synchronize()
        grads[which] = {n: t.grad for n, t in inputs.items()}
    position = "xyz" if kind == "leaf" else "means3D"
    assert float(grads["small"][position].abs().max()) > 0, "the loss reaches no Gaussian"
    for n, g in grads["small"].items():
        big = grads["large"][n]
        assert (g is None) == (big is None), f"{n}: {'no ' if g is None else ''}gradient from the small set, the opposite from the large"
        if g is not None:
            ne = int((g != big).sum())
            print(f"{kind} {output} {n}: {ne} of {g.numel()} differ, max |d| = {float((g - big).abs().max()):.3e}")
            assert torch.equal(g, big), f"dL/d{n} of a loss on {output} alone depends on the outputs that took no part"
    if output != "feature_map":   # (no gradient reached the map: its pass is skipped)
        assert grads["large"]["features"] is None


def _camera_model(cam):
    W, H = cam.image_width, cam.image_height
    return ("pinhole", 0.9 * W / (2 * cam.tanfovx), 0.95 * H / (2 * cam.tanfovy), 0.5 * W + 1.3, 0.5 * H - 0.7)


# camera kind -> (keywords but for the tensor, the tied inputs)
CAMERA_KINDS = {
    "cam": (dict(camera_grads=True), ("viewmatrix", "projmatrix", "campos")),
    "cm_true": (dict(camera_model_grads=True), ("viewmatrix", "campos")),
    "cm_tensor": ({}, ("viewmatrix", "campos", "intrinsics")),
}


@pytest.mark.parametrize("camera", list(CAMERA_KINDS))
@pytest.mark.parametrize("kind", ["plain", "leaf"])
def test_camera_routing(kind, camera, monkeypatch):
    """Exactly one of the tied camera inputs requires a gradient, then none: that one gets a gradient of its own shape, the others
    None; with none, the camera target is not even allocated."""
    from diff_gaussian_rasterization import _C
    scene, cam, _, up = _scene()
    reference_outputs(kind)
    calls = []
    for helper in CAMERA_TARGET_HELPERS:
        def spy(*a, _orig=getattr(_C, helper), **kw):
            calls.append(a)
            return _orig(*a, **kw)
        monkeypatch.setattr(_C, helper, spy)
    opts, tied = CAMERA_KINDS[camera]
    cm = _camera_model(cam)
    if camera != "cam":
        opts = dict(opts, camera_model=cm)
    for needy in tied + (None,):
        st = _settings(scene, cam)
        tensors = {n: getattr(st, n).clone().requires_grad_(n == needy) for n in ("viewmatrix", "projmatrix", "campos")}
        if camera == "cm_tensor":
            tensors["intrinsics"] = torch.tensor(cm[1:], device=DEV).requires_grad_(needy == "intrinsics")
            opts = dict(opts, camera_model_grads=tensors["intrinsics"])
        del calls[:]
        outs, inputs = render(kind, dict(opts, depth_alpha="depth"), settings=st._replace(**{n: tensors[n] for n in st._fields if n in tensors}))
        res = named(outs, ("depth", "alpha"), False)
        sum((res[n] * up[n]).sum() for n in ("color", "depth", "alpha")).backward()
        torch.cuda.synchronize()
        assert len(calls) == (0 if needy is None else 1), f"{needy}: the camera target was built {len(calls)} times"
        for n, t in tensors.items():
            if n == needy:
                assert t.grad is not None and t.grad.shape == t.shape and float(t.grad.abs().max()) > 0, n
            else:
                assert t.grad is None, f"{n} got a gradient while {needy} alone requires one"
        for n, t in inputs.items():
            assert t.grad is not None and t.grad.shape == t.shape, n


@pytest.mark.parametrize("kind", ["plain", "leaf"])
def test_no_camera_option_ties_no_camera_tensor(kind, monkeypatch):
    """Without camera_grads / camera_model_grads a viewmatrix that requires a gradient is no input: it neither makes the outputs
    require one nor gets one."""
    from diff_gaussian_rasterization import _C
    scene, cam, _, up = _scene()
    calls = []
    for helper in CAMERA_TARGET_HELPERS:
        monkeypatch.setattr(_C, helper, lambda *a, **kw: calls.append(a))
    for opts in ({}, dict(camera_model=_camera_model(cam))):
        st = _settings(scene, cam)
        st = st._replace(viewmatrix=st.viewmatrix.clone().requires_grad_(True), campos=st.campos.clone().requires_grad_(True))
        outs, _ = render(kind, opts, settings=st, gaussians_require_grad=False)
        assert not any(o.requires_grad for o in outs)
        outs, inputs = render(kind, opts, settings=st)
        (outs[0] * up["color"]).sum().backward()
        torch.cuda.synchronize()
        assert st.viewmatrix.grad is None and st.campos.grad is None and not calls
        assert all(t.grad is not None for t in inputs.values())
