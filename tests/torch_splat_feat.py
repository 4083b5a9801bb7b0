"""The float64 dense autograd restatement of the rasterizer forward with K per-Gaussian feature channels blended beside the colours:
feature_map[k](p) = sum_i features[i][k] alpha_i T_i(p) with the image's own alpha and T, no background term.  TEST INFRASTRUCTURE,
the feature counterpart of tests/torch_splat.py, with the same conventions and the same deliberate deviations (straight-through 0.99
clamp; inside the frustum clamp of the EWA Jacobian the clamped t.x / t.y are constants; masks, tile membership, depth order, culling
and radii carry no gradient; discrete decisions from the oracle state `o` of the same inputs).  Gradients come from torch.autograd,
so agreement with the HIP feature passes (csrc/features.hip) checks their hand-written formulas rather than a copy of them.

The weights of a pixel do not depend on what is blended with them, so the channels are blended by the dense blend of
tests/torch_splat_cam.py itself, three at a time in the place of a precomputed colour on a zero background -- inside ONE autograd
graph over the same leaves (and the same camera tensors, shared or one copy per Gaussian: camera_terms() below)."""
import torch

import torch_splat_cam


def render(o, means3D, scales, rotations, opacities, shs, features, V=None, PM=None, campos=None, dtype=torch.float64, **kw):
    """-> (image (3,H,W) [, depth (H,W), alpha (H,W) with depth_mode=], feature_map (K,H,W)).  V, PM, campos: the camera tensors,
    default the oracle state's; **kw: the keywords of torch_splat_cam.render (antialiasing, depth_mode, scale_modifier)."""
    W, H = o["W"], o["H"]
    cam = [torch.from_numpy(o[k]).reshape(s) if t is None else t
           for k, s, t in (("viewmatrix", (4, 4), V), ("projmatrix", (4, 4), PM), ("campos", (3,), campos))]
    out = torch_splat_cam.render(o, means3D, scales, rotations, opacities, shs, *cam, dtype=dtype, **kw)
    out = out if isinstance(out, tuple) else (out,)
    black = dict(o, bg=o["bg"] * 0)
    feat_kw = {k: v for k, v in kw.items() if k != "depth_mode"}
    K = features.shape[1]
    maps = []
    for k0 in range(0, K, 3):
        f3 = features[:, k0:k0 + 3].to(dtype)
        if f3.shape[1] < 3:
            f3 = torch.cat([f3, torch.zeros(f3.shape[0], 3 - f3.shape[1], dtype=dtype)], 1)
        m = torch_splat_cam.render(black, means3D, scales, rotations, opacities, None, *cam, colors_precomp=f3, dtype=dtype, **feat_kw)
        maps.append(m[:min(3, K - k0)])
    return (*out, torch.cat(maps, 0).reshape(K, H, W))


def camera_terms(o, inputs, features, dL, **kw):
    """torch_splat_cam.camera_terms() for the loss sum(outputs * dL) over render()'s outputs, the feature map included (dL: one
    tensor per output, the map's last) -> (total, abs_total, d32) over "V", "PM", "campos"."""
    P = inputs["means3D"].shape[0]
    out = {}
    for dt in (torch.float64, torch.float32):
        cam = {"V": inputs["V"].to(dt).expand(P, 4, 4).clone().requires_grad_(True),
               "PM": inputs["PM"].to(dt).expand(P, 4, 4).clone().requires_grad_(True),
               "campos": inputs["campos"].to(dt).expand(P, 3).clone().requires_grad_(True)}
        res = render(o, inputs["means3D"], inputs["scales"], inputs["rotations"], inputs["opacities"], inputs["shs"], features,
                     cam["V"], cam["PM"], cam["campos"], dtype=dt, **kw)
        loss = sum((r * d.to(dt).reshape(r.shape)).sum() for r, d in zip(res, dL))
        grads = torch.autograd.grad(loss, list(cam.values()), allow_unused=True)
        out[dt] = {k: (torch.zeros_like(cam[k]) if g is None else g).to(torch.float64) for k, g in zip(cam, grads)}
    total = {k: v.sum(0) for k, v in out[torch.float64].items()}
    abs_total = {k: v.abs().sum(0) for k, v in out[torch.float64].items()}
    d32 = {k: float((out[torch.float32][k].sum(0) - total[k]).abs().max()) for k in total}
    return total, abs_total, d32
