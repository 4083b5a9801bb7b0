"""CPU, no library: one bad value per public keyword, fed to every entry point that has the keyword -- GaussianRasterizer(...)(...),
rasterize_gaussians, rasterize_gaussians_depth_alpha and fused_params.rasterize_leaf_gaussians.  Each must be refused before anything
runs (the tensors are on the CPU, so anything that ran would fail differently), with the documented exception type, and every entry
point must raise the same type and message as every other."""
import inspect

import pytest
import torch

import __graft_entry__  # noqa: F401

P, W, H = 4, 16, 8
PINHOLE = ("pinhole", 10.0, 10.0, 8.0, 4.0)
DEPTH = dict(depth_alpha="depth")
# (id, the keywords of the bad call, the documented exception, entry points the row does not apply to)
TABLE = [
    ("depth_alpha_unknown", dict(depth_alpha="range"), ValueError, ()),
    ("antialiasing_not_bool", dict(antialiasing=1), TypeError, ()),
    ("camera_grads_not_bool", dict(camera_grads="yes"), TypeError, ()),
    ("distortion_not_bool", dict(DEPTH, distortion=1), TypeError, ()),
    ("median_depth_not_bool", dict(DEPTH, median_depth="yes"), TypeError, ()),
    # (rasterize_gaussians_depth_alpha cannot be called without a mode)
    ("distortion_without_mode", dict(depth_alpha=None, distortion=True), ValueError, ("rasterize_gaussians_depth_alpha",)),
    ("median_depth_without_mode", dict(depth_alpha=None, median_depth=True), ValueError, ("rasterize_gaussians_depth_alpha",)),
    ("camera_model_not_5_tuple", dict(camera_model=("pinhole", 10.0)), TypeError, ()),
    ("camera_model_unknown", dict(camera_model=("box", 10.0, 10.0, 8.0, 4.0)), ValueError, ()),
    ("camera_model_bad_focal", dict(camera_model=("fisheye", -1.0, 10.0, 8.0, 4.0)), ValueError, ()),
    ("camera_grads_with_model", dict(camera_grads=True, camera_model=PINHOLE), NotImplementedError, ()),
    ("camera_model_grads_without_model", dict(camera_model_grads=True), ValueError, ()),
    ("camera_model_grads_not_tensor", dict(camera_model=PINHOLE, camera_model_grads="yes"), TypeError, ()),
    ("camera_model_grads_wrong_shape", dict(camera_model=PINHOLE, camera_model_grads=torch.zeros(3)), ValueError, ()),
    ("camera_model_grads_wrong_dtype", dict(camera_model=PINHOLE, camera_model_grads=torch.zeros(4, dtype=torch.float64)), ValueError, ()),
    ("absgrad_not_2_tuple", dict(absgrad=(None,)), TypeError, ()),
    ("absgrad_both_none", dict(absgrad=(None, None)), ValueError, ()),
    ("index_maps_not_3_tuple", dict(index_maps=(None, None)), TypeError, ()),
    ("index_maps_wrong_dtype", dict(index_maps=(torch.zeros(H, W), None, None)), ValueError, ()),
    ("contrib_stats_all_none", dict(contrib_stats=(None, None, None)), RuntimeError, ()),
    ("contrib_stats_wrong_shape", dict(contrib_stats=(torch.zeros(P + 1), None, None)), RuntimeError, ()),
    ("features_not_tensor", dict(features=[1.0]), TypeError, ()),
    ("features_wrong_dtype", dict(features=torch.zeros(P, 2, dtype=torch.float64)), RuntimeError, ()),
    ("features_sh", dict(features=torch.zeros(P, 4, 2)), NotImplementedError, ()),
]


def _entry_points():
    """name -> (callable taking keywords only, the keywords it has)"""
    import diff_gaussian_rasterization as dgr
    import fused_params
    st = dgr.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=1.0, tanfovy=0.5, bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=torch.eye(4),
        projmatrix=torch.eye(4), sh_degree=0, campos=torch.zeros(3), prefiltered=False, debug=False)
    z = torch.zeros
    empty = torch.Tensor([])

    def module(features=None, **kw):
        return dgr.GaussianRasterizer(st, **kw)(means3D=z(P, 3), means2D=z(P, 3), opacities=z(P, 1), shs=z(P, 1, 3), scales=z(P, 3),
                                                rotations=z(P, 4), features=features)

    def packed(**kw):
        return dgr.rasterize_gaussians(z(P, 3), z(P, 3), z(P, 1, 3), empty, z(P, 1), z(P, 3), z(P, 4), empty, st, **kw)

    def packed_maps(depth_alpha="depth", **kw):
        return dgr.rasterize_gaussians_depth_alpha(z(P, 3), z(P, 3), z(P, 1, 3), empty, z(P, 1), z(P, 3), z(P, 4), empty, st,
                                                   depth_alpha, **kw)

    def leaf(**kw):
        return fused_params.rasterize_leaf_gaussians(z(P, 3), z(P, 3), z(P, 1, 3), z(P, 0, 3), z(P, 1), z(P, 3), z(P, 4), st, **kw)

    keywords = lambda f: set(inspect.signature(f).parameters)
    return {"GaussianRasterizer": (module, (keywords(dgr.GaussianRasterizer.__init__) | {"features"}) - {"self", "raster_settings"}),
            "rasterize_gaussians": (packed, keywords(dgr.rasterize_gaussians)),
            "rasterize_gaussians_depth_alpha": (packed_maps, keywords(dgr.rasterize_gaussians_depth_alpha)),
            "rasterize_leaf_gaussians": (leaf, keywords(fused_params.rasterize_leaf_gaussians))}


def refusals(kw, skip=()):
    """entry point -> (exception type name, message) of the call with `kw`, for every entry point that has these keywords"""
    out = {}
    for name, (call, has) in _entry_points().items():
        if name in skip or not set(kw) <= has:
            continue
        try:
            call(**kw)
            out[name] = ("no exception", "")
        except Exception as e:   # noqa: BLE001  (the table records whatever is raised)
            out[name] = (type(e).__name__, str(e))
    return out


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_every_entry_point_refuses_alike(row):
    _, kw, exc, skip = row
    got = refusals(kw, skip)
    assert len(got) >= 2 and "GaussianRasterizer" in got and "rasterize_leaf_gaussians" in got, sorted(got)
    for name, (typ, msg) in got.items():
        assert typ == exc.__name__, f"{name}: {typ}: {msg}"
        assert msg, name
    assert len(set(got.values())) == 1, got


def test_valid_keywords_reach_the_render():
    """the table's base call is valid: what refuses it is the render itself, which has no CPU path"""
    for name, (typ, msg) in refusals({}).items():
        assert typ == "RuntimeError" and "HIP (cuda) tensor" in msg, (name, typ, msg)


if __name__ == "__main__":   # the table as text: one line per entry point
    for rid, kw, _, skip in TABLE:
        for name, (typ, msg) in refusals(kw, skip).items():
            print(f"{rid} | {name} | {typ} | {msg}")
