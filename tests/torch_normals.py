"""Float64 autograd restatement of include/gsr_normals.h: the per-Gaussian normals, the depth normals (2DGS's depth_to_normal in view
space, written as the header defines it: unproject, two central differences, cross product, normalise) and the normal-consistency
loss.  Plain torch on whatever device the inputs live on; the discrete decisions -- the axis of the smallest scale, the facing sign,
which depths are valid -- are made from the float32 input values, the arithmetic in `dtype` (float64; float32 gives "the same formula
evaluated by torch in fp32", the yardstick of the widened bar in test_normals_gpu.py)."""
import numpy as np
import torch


def rotation_matrix(qn):
    """(P, 3, 3) of unit quaternions (w, x, y, z): gsr_model.build_rotation's entries"""
    w, x, y, z = qn.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)


def min_axis(scales):
    """index of the smallest scale under a strict <: the first index wins an exact tie"""
    s = scales.detach()
    k = torch.zeros(s.shape[0], dtype=torch.long, device=s.device)
    m = s[:, 0].clone()
    for j in (1, 2):
        less = s[:, j] < m
        k = torch.where(less, torch.full_like(k, j), k)
        m = torch.where(less, s[:, j], m)
    return k


def gaussian_normals(scales, rotations, means3D, viewmatrix, space="view", dtype=torch.float64, parts=False):
    """-> (P, 3); parts=True: (normals, k, sign, n_v . t / |t| before the flip)"""
    k = min_axis(scales)
    q, m, V = rotations.to(dtype), means3D.to(dtype), viewmatrix.to(dtype).reshape(4, 4)
    sq = q.pow(2).sum(1)
    zero = sq == 0                                                        # no normal and no gradient (the square root is kept away from 0)
    qn = q / torch.where(zero, torch.ones_like(sq), sq).sqrt()[:, None]
    R = rotation_matrix(qn)
    n_w = R[torch.arange(q.shape[0], device=q.device), :, k]
    n_w = torch.where(zero[:, None], torch.zeros_like(n_w), n_w)
    t = m @ V[:3, :3] + V[3, :3]
    n_v = n_w @ V[:3, :3]
    facing = (n_v * t).sum(1).detach()
    sign = torch.where(facing > 0, -torch.ones_like(facing), torch.ones_like(facing))
    out = sign[:, None] * (n_v if space == "view" else n_w)
    if parts:
        return out, k, sign, facing / t.detach().norm(dim=1)
    return out


def _valid(z):
    return torch.isfinite(z) & (z > 0)


def depth_normals(depth, tanfovx, tanfovy, dtype=torch.float64):
    """depth (H, W) or (1, H, W) -> (3, H, W).  tanfovx / tanfovy are taken at float32 precision, as the kernels receive them."""
    z = depth.reshape(depth.shape[-2], depth.shape[-1])
    H, W = z.shape
    tx, ty = float(np.float32(tanfovx)), float(np.float32(tanfovy))
    ok = _valid(z.detach())
    z = torch.where(ok, z.to(dtype), torch.ones((), dtype=dtype, device=z.device))   # invalid depths never enter a valid normal
    out = torch.zeros(3, H, W, dtype=dtype, device=z.device)
    if H < 3 or W < 3:
        return out + 0 * z.sum()
    X = ((2 * torch.arange(W, dtype=dtype, device=z.device) + 1) / W - 1) * tx
    Y = ((2 * torch.arange(H, dtype=dtype, device=z.device) + 1) / H - 1) * ty
    Pt = torch.stack((X[None, :] * z, Y[:, None] * z, z))                        # (3, H, W)
    a = Pt[:, 2:, 1:-1] - Pt[:, :-2, 1:-1]                                         # P(x, y + 1) - P(x, y - 1)
    b = Pt[:, 1:-1, 2:] - Pt[:, 1:-1, :-2]                                         # P(x + 1, y) - P(x - 1, y)
    c = torch.cross(a, b, dim=0)
    n = c / c.norm(dim=0, keepdim=True).clamp_min(1e-12)
    good = ok[2:, 1:-1] & ok[:-2, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2]
    inner = torch.where(good[None], n, torch.zeros_like(n))
    return torch.nn.functional.pad(inner, (1, 1, 1, 1))


def normal_consistency_loss(normal_map, depth, alpha, tanfovx, tanfovy, dtype=torch.float64):
    n_d = depth_normals(depth, tanfovx, tanfovy, dtype)
    a = 1.0 if alpha is None else alpha.detach().to(dtype).reshape(n_d.shape[1:])
    return (1 - a * (normal_map.to(dtype) * n_d).sum(0)).mean()


# ---- inputs shared by the CPU and the GPU tests ------------------------------------------------------------------------------------
def plane_depth(W, H, tanx, tany, p0=(0.0, 0.0, 4.0), normal=(0.3, -0.2, -1.0)):
    """view-space z of the plane through p0 with the given normal at every pixel centre (float64), and the unit normal"""
    n = torch.tensor(normal, dtype=torch.float64)
    X = ((2 * torch.arange(W, dtype=torch.float64) + 1) / W - 1) * float(np.float32(tanx))
    Y = ((2 * torch.arange(H, dtype=torch.float64) + 1) / H - 1) * float(np.float32(tany))
    z = float(n @ torch.tensor(p0, dtype=torch.float64)) / (n[0] * X[None, :] + n[1] * Y[:, None] + n[2])
    return z, n / n.norm()
