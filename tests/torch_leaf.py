"""The leaf-activation backward of the per-Gaussian pass (csrc/gaussian_backward_tail.inc) written out in torch: the float64 reference
of tests/test_leaf_reference_cpu.py and tests/test_gaussian_pass_gpu.py, the stock float32 chain their bar is scaled by, the
normalised error both are measured with, and the raw leaves those tests share.  Plain torch, no project code.

    opacity  = sigmoid(l)      d/dl  = g s(l) (1 - s(l))
    scaling  = exp(x)          d/dx  = g exp(x)
    rotation = q / d           d/dq  = g / d - q (q . g) / d^3,  d = max(|q|, 1e-12); where the clamp is active d is a constant
                                       and the radial term is absent (torch.nn.functional.normalize)
"""
import math

import torch

NORM_EPS = 1e-12   # torch.nn.functional.normalize's eps
FLOOR = 2.0 ** -22


# ---- (a) the float64 reference ------------------------------------------------------------------------------------------------
def jacobians(opacity, scaling, rotation):
    """-> (J_opacity (P,1), J_scaling (P,3), d (P,1)) in float64, taken from the raw leaves in float64"""
    l, x, q = opacity.double(), scaling.double(), rotation.double()
    s = torch.sigmoid(l)
    # (1 - s in float64 keeps 2^-53 / (1 - s) relative: 1.3e-10 at a logit of 14, the largest the bars are held at)
    return s * (1 - s), torch.exp(x), q.norm(dim=-1, keepdim=True).clamp_min(NORM_EPS)


def reference(opacity, scaling, rotation, g_opacity, g_scaling, g_rotation):
    """J^T g_act in float64 -> dict(opacity (P,1), scaling (P,3), rotation (P,4))"""
    Jo, Js, d = jacobians(opacity, scaling, rotation)
    q, g = rotation.double(), g_rotation.double()
    radial = torch.where(q.norm(dim=-1, keepdim=True) > NORM_EPS, q * (q * g).sum(-1, keepdim=True) / d ** 3, torch.zeros_like(q))
    return dict(opacity=g_opacity.double() * Jo, scaling=g_scaling.double() * Js, rotation=g / d - radial)


def autograd_reference(opacity, scaling, rotation, g_opacity, g_scaling, g_rotation):
    """The same through torch.autograd over float64 activations (what (a) is checked against)"""
    leaves = [t.double().clone().requires_grad_(True) for t in (opacity, scaling, rotation)]
    act = (torch.sigmoid(leaves[0]), torch.exp(leaves[1]), torch.nn.functional.normalize(leaves[2], dim=-1))
    grads = torch.autograd.grad(act, leaves, [g.double() for g in (g_opacity, g_scaling, g_rotation)])
    return dict(zip(("opacity", "scaling", "rotation"), grads))


# ---- (b) the stock fp32 chain -------------------------------------------------------------------------------------------------
def stock(opacity, scaling, rotation, g_opacity, g_scaling, g_rotation):
    """What stock PyTorch computes in float32 on the tensors' device: sigmoid backward g (1 - y) y, exp backward g y, autograd
    through F.normalize"""
    l, x, g_o, g_s, g_r = (t.float() for t in (opacity, scaling, g_opacity, g_scaling, g_rotation))
    y = torch.sigmoid(l)
    q = rotation.float().clone().requires_grad_(True)
    (d_q,) = torch.autograd.grad(torch.nn.functional.normalize(q, dim=-1), q, g_r)
    return dict(opacity=g_o * (1 - y) * y, scaling=g_s * torch.exp(x), rotation=d_q)


# ---- (c) the normalised error -------------------------------------------------------------------------------------------------
def normalised_error(got, ref, opacity, scaling, rotation, g_opacity, g_scaling, g_rotation):
    """per Gaussian, float64 (P,) for each leaf: max over the elements of |got - ref| / (|g| |J|) for opacity and scaling,
    ||got - ref|| / (||g|| / d) for the rotation.  Elements (rows, for the rotation) with g == 0 must have got == 0 -- asserted --
    and count as 0."""
    Jo, Js, d = (t.to(ref["opacity"].device) for t in jacobians(opacity, scaling, rotation))
    out = {}
    for name, J, g in (("opacity", Jo, g_opacity), ("scaling", Js, g_scaling)):
        g = g.double().to(J.device)
        e = (got[name].double() - ref[name]).abs()
        zero = g == 0
        assert bool((got[name][zero] == 0).all()), f"{name}: a non-zero gradient where g_act is zero"
        out[name] = torch.where(zero, torch.zeros_like(e), e / torch.where(zero, torch.ones_like(g), g.abs() * J)).amax(dim=1)
    g = g_rotation.double().to(d.device)
    gn = g.norm(dim=-1)
    zero = (g == 0).all(dim=-1)
    assert bool((got["rotation"][zero] == 0).all()), "rotation: a non-zero gradient where g_act is zero"
    e = (got["rotation"].double() - ref["rotation"]).norm(dim=-1)
    out["rotation"] = torch.where(zero, torch.zeros_like(e), e / torch.where(zero, torch.ones_like(gn), gn / d[:, 0]))
    return out


# ---- the fixtures -------------------------------------------------------------------------------------------------------------
ROW_ZERO_QUAT, ROW_UNIT_QUAT, ROW_LOGIT_PLUS20, ROW_LOGIT_MINUS20, ROW_BIG = 5, 6, 7, 8, 9
BANDS = ((0.0, 4.0), (4.0, 8.0), (8.0, 14.0))   # |logit|


def fixture_a(P=257, rest=15, seed=0):
    """Raw leaves of fixture A for a camera at (0, 0, -4) looking down +z -> [xyz (P,3), features_dc (P,1,3), features_rest
    (P,rest,3), opacity (P,1), scaling (P,3), rotation (P,4)], float32.
    Logits: a third each with |l| in [0, 4], [4, 8] and [8, 14]; rows 7 and 8 at +20 and -20.  The saturated-positive splats are
    opaque, so the sign is mostly positive in the far half of the scene and mostly negative in the near half: an opaque wall in
    front would leave nothing behind it with a gradient.
    Log-scales in [-9, 1], each element drawn on its own (mixed within a Gaussian), most of them small so that the image is not
    covered by a few splats; row 9 is one large, faint splat (the cooperative slot sum).
    Quaternions: random directions, norms log-uniform in [1e-3, 1e3]; row 5 exactly zero, row 6 of norm 1 to within an ulp.
    One row in six lies behind the camera's near plane (culled); rows 5 to 9 and the last row lie in front of it."""
    g = torch.Generator().manual_seed(4000 + seed)
    u = lambda *s: torch.rand(*s, generator=g)
    xyz = torch.stack([2.4 * u(P) - 1.2, 1.8 * u(P) - 0.9, 3.0 * u(P) - 1.5], dim=1)
    behind = torch.arange(P) % 6 == 3
    behind[[ROW_ZERO_QUAT, ROW_UNIT_QUAT, ROW_LOGIT_PLUS20, ROW_LOGIT_MINUS20, ROW_BIG, P - 1]] = False
    xyz[behind, 2] = -4.5 - u(int(behind.sum()))
    dc = torch.randn(P, 1, 3, generator=g)
    fr = 0.2 * torch.randn(P, rest, 3, generator=g)
    band = torch.randperm(P, generator=g) % 3
    lo = torch.tensor([b[0] for b in BANDS])[band]
    hi = torch.tensor([b[1] for b in BANDS])[band]
    mag = lo + (hi - lo) * u(P)
    p_pos = torch.where(band == 0, torch.full((P,), 0.5), 0.15 + 0.7 * ((xyz[:, 2] + 1.5) / 3.0).clamp(0, 1))
    opacity = (torch.where(u(P) < p_pos, mag, -mag))[:, None].contiguous()
    kind = u(P, 3)
    scaling = torch.where(kind < 0.25, -9.0 + 4.0 * u(P, 3), torch.where(kind < 0.9, -5.0 + 2.0 * u(P, 3), -3.0 + 4.0 * u(P, 3)))
    q = torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=-1)
    rotation = q * torch.exp(math.log(1e3) * (2 * u(P, 1) - 1))
    # the named rows: in front of everything else, small, so that they are seen and have a gradient
    for k, row in enumerate((ROW_ZERO_QUAT, ROW_UNIT_QUAT, ROW_LOGIT_PLUS20, ROW_LOGIT_MINUS20)):
        xyz[row] = torch.tensor([-0.6 + 0.4 * k, 0.3 - 0.2 * k, -1.9])
        scaling[row] = torch.tensor([-3.0, -3.5, -2.5])
    rotation[ROW_ZERO_QUAT] = 0.0
    rotation[ROW_UNIT_QUAT] = q[ROW_UNIT_QUAT]
    opacity[ROW_ZERO_QUAT, 0], opacity[ROW_UNIT_QUAT, 0] = 1.0, -1.0
    opacity[ROW_LOGIT_PLUS20, 0], opacity[ROW_LOGIT_MINUS20, 0] = 20.0, -20.0
    xyz[ROW_BIG] = torch.tensor([0.1, -0.1, 0.5])
    scaling[ROW_BIG] = torch.tensor([0.0, -0.5, -6.0])
    opacity[ROW_BIG, 0] = -2.0
    xyz[P - 1] = torch.tensor([0.7, -0.5, -1.8])
    scaling[P - 1] = torch.tensor([-2.5, -3.0, -4.0])
    opacity[P - 1, 0] = 6.0
    return [t.contiguous() for t in (xyz, dc, fr, opacity, scaling, rotation)]


PARTS_B = ((0, 64), (64, 1), (128, 77), (256, 77))   # (first, count) of fixture B; the last ends the scene in mid-wave


def fixture_b(P=333, rest=15, seed=0):
    """Raw leaves of fixture B, benign values: logits in [-2, 4], log-scales around -3, quaternion norms in [0.5, 2]; one row in
    five lies behind the near plane; row 64 lies in front of it."""
    g = torch.Generator().manual_seed(5000 + seed)
    u = lambda *s: torch.rand(*s, generator=g)
    xyz = torch.stack([2.4 * u(P) - 1.2, 1.8 * u(P) - 0.9, 3.0 * u(P) - 1.5], dim=1)
    behind = torch.arange(P) % 5 == 2
    behind[64] = False
    xyz[behind, 2] = -4.5 - u(int(behind.sum()))
    dc = torch.randn(P, 1, 3, generator=g)
    fr = 0.2 * torch.randn(P, rest, 3, generator=g)
    opacity = -2.0 + 6.0 * u(P, 1)
    scaling = -3.0 + 0.7 * torch.randn(P, 3, generator=g)
    rotation = torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=-1) * (0.5 + 1.5 * u(P, 1))
    return [t.contiguous() for t in (xyz, dc, fr, opacity, scaling, rotation)]


def upstream(W, H, seed=1):
    """dL/dpixel (3,H,W) of the tests that share the fixtures"""
    return torch.randn(3, H, W, generator=torch.Generator().manual_seed(seed))


def activated(leaves):
    """the five tensors the rasterizer takes, by stock torch in the leaves' dtype and on their device"""
    xyz, dc, fr, opacity, scaling, rotation = leaves
    return dict(means3D=xyz, shs=torch.cat((dc, fr), dim=1).contiguous(), opacities=torch.sigmoid(opacity),
                scales=torch.exp(scaling), rotations=torch.nn.functional.normalize(rotation, dim=-1))
