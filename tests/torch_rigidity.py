"""PyTorch restatement of fused_rigidity (include/gsr_rigidity.h): the rigidity, rotation and isometry losses of Dynamic 3D Gaussians
(Luiten et al., 3DV 2024, get_loss: weighted_l2_loss_v1 / _v2, quat_mult, build_rotation) over a K-NN table with holes (-1).

    (a) loss_terms       the plain sequence, which autograd differentiates; in float64 the reference, in float32 the stock sequence
    (b) analytic_grads   the contribution of every edge to its centre row and to its neighbour row in closed form, float64, summed per
                         row in the kernels' order (the centre's edges in ascending k, then the incoming edges in ascending edge id:
                         index_add_ on the CPU adds sequentially), and the per-row scale S_j: the float64 sum of the norms of every
                         contribution that is added into row j

For a valid edge (i, k), j = idx[i, k] >= 0:  q = r / |r|, rel = q (x) p (Hamilton product, w first), R = build_rotation(rel),
c = x_j - x_i, rigid = sqrt(w |R^T c - o|^2 + 1e-20), rot = sqrt(w |rel_j - rel_i|^2 + 1e-20),
iso = sqrt(w (sqrt(|c|^2 + 1e-20) - d)^2 + 1e-20); every term is the sum over the valid edges divided by their number N_e.
The tables are looked at only where idx >= 0: what the other places hold (NaN included) is replaced by 0 first.
"""
import numpy as np
import torch

import torch_knn

EPS = 1e-20
SIDES = {63: 0.10, 257: 0.15, 1000: 0.25, 4097: 0.40}   # cube side per cloud size: most weights exp(-2000 d^2) stay above 1e-3
LAMBDAS = (4.0, 4.0, 2.0)


def quat_mult(a, b):
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2,
                        w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                        w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], dim=-1)


def quat_conj(q):
    return q * q.new_tensor([1.0, -1.0, -1.0, -1.0])


def rotation_of_unit(v):
    """(..., 4) unit quaternion (w, x, y, z) -> (..., 3, 3), the library's convention"""
    r, x, y, z = v.unbind(-1)
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
            2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
            2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=-1).reshape(v.shape[:-1] + (3, 3))


def build_rotation(r):
    return rotation_of_unit(r / torch.sqrt((r * r).sum(-1, keepdim=True)))


# ---- clouds and tables ---------------------------------------------------------------------------------------------------------
def make_cloud(P, seed=0, side=None):
    """-> (xyz0 (P, 3) uniform in a cube of side SIDES[P], rot0 (P, 4) unit quaternions with normal components), float32"""
    side = SIDES[P] if side is None else side
    g = torch.Generator().manual_seed(1000 + 7 * P + seed)
    xyz0 = (torch.rand(P, 3, generator=g, dtype=torch.float64) * side).float()
    rot0 = torch.randn(P, 4, generator=g, dtype=torch.float64)
    return xyz0, (rot0 / rot0.norm(dim=1, keepdim=True)).float()


def perturb(xyz0, rot0, side, seed=0):
    """the current leaves: normal noise of 1 % of the side on xyz and of 0.05 on the quaternion components (left unnormalised)"""
    g = torch.Generator().manual_seed(5000 + seed)
    xyz = xyz0.double() + 0.01 * side * torch.randn(xyz0.shape, generator=g, dtype=torch.float64)
    rot = rot0.double() + 0.05 * torch.randn(rot0.shape, generator=g, dtype=torch.float64)
    return xyz.float(), rot.float()


def capture(xyz0, rot0, K, weight_lambda=2000.0, mask=None):
    """the tables RigidityState.capture builds, float32 on the CPU: idx, prev_offset, prev_dist, weight, prev_inv_rot; zeros at -1"""
    P = xyz0.shape[0]
    rows = torch.arange(P) if mask is None else torch.nonzero(mask).flatten()
    d2s, ids = torch_knn.knn(xyz0[rows].numpy(), K)
    ids = torch.from_numpy(ids).long()
    idx = torch.full((P, K), -1, dtype=torch.int32)
    idx[rows] = torch.where(ids >= 0, rows[ids.clamp(min=0)], ids).int()
    valid = idx >= 0
    dist2 = torch.zeros((P, K), dtype=torch.float32)
    dist2[rows] = torch.from_numpy(d2s)
    dist2 = torch.where(valid, dist2, torch.zeros(()))
    off = torch.where(valid[..., None], xyz0[idx.long().clamp(min=0)] - xyz0[:, None], torch.zeros(()))
    weight = torch.where(valid, torch.exp(-weight_lambda * dist2), torch.zeros(()))
    q0 = rot0 / rot0.norm(dim=1, keepdim=True)
    return {"idx": idx, "prev_offset": off.contiguous(), "prev_dist": torch.sqrt(dist2), "weight": weight, "prev_inv_rot": quat_conj(q0).contiguous()}


def strong_share(t, floor=1e-3):
    """the share of the valid edges whose weight is at least `floor`"""
    valid = t["idx"] >= 0
    return float((t["weight"][valid] >= floor).double().mean())


def _tables(t, dtype):
    idx = t["idx"].long()
    valid = idx >= 0
    z = torch.zeros((), dtype=dtype)
    o = torch.where(valid[..., None], t["prev_offset"].to(dtype), z)
    d = torch.where(valid, t["prev_dist"].to(dtype), z)
    w = torch.where(valid, t["weight"].to(dtype), z)
    return idx.clamp(min=0), valid, o, d, w, t["prev_inv_rot"].to(dtype)


# ---- (a) the plain sequence ----------------------------------------------------------------------------------------------------
def loss_terms(xyz, rotation, t, dtype=torch.float64):
    """-> (rigid, rot, iso) scalars of `dtype`, differentiable w.r.t. xyz and rotation"""
    j, valid, o, d, w, p = _tables(t, dtype)
    x, r = xyz.to(dtype), rotation.to(dtype)
    q = r / torch.sqrt((r * r).sum(-1, keepdim=True))
    rel = quat_mult(q, p)
    R = build_rotation(rel)
    c = x[j] - x[:, None]
    u = (R.transpose(2, 1)[:, None] @ c[:, :, :, None]).squeeze(-1)
    rigid = torch.sqrt(((u - o) ** 2).sum(-1) * w + EPS)
    rot = torch.sqrt(((rel[j] - rel[:, None]) ** 2).sum(-1) * w + EPS)
    mag = torch.sqrt((c ** 2).sum(-1) + EPS)
    iso = torch.sqrt(((mag - d) ** 2) * w + EPS)
    ne = int(valid.sum())
    zero = torch.zeros((), dtype=dtype)
    if ne == 0:
        return tuple((x.sum() + r.sum()) * 0 for _ in range(3))
    return tuple(torch.where(valid, term, zero).sum() / ne for term in (rigid, rot, iso))


def loss_and_grads(xyz, rotation, t, lambdas=LAMBDAS, dtype=torch.float64):
    """autograd of (a) -> (values (4,): total, rigid, rot, iso; grad_xyz (P, 3); grad_rot (P, 4)) in `dtype`"""
    x = xyz.detach().to(dtype).requires_grad_(True)
    r = rotation.detach().to(dtype).requires_grad_(True)
    terms = loss_terms(x, r, t, dtype)
    total = lambdas[0] * terms[0] + lambdas[1] * terms[1] + lambdas[2] * terms[2]
    gx, gr = torch.autograd.grad(total, (x, r), allow_unused=True)
    gx = torch.zeros_like(x) if gx is None else gx
    gr = torch.zeros_like(r) if gr is None else gr
    return torch.stack([total.detach()] + [v.detach() for v in terms]), gx, gr


# ---- (b) closed form per edge ----------------------------------------------------------------------------------------------------
def _fold(G, v):
    """dL/dR as G[..., b, a] = dL/dR[b][a] -> dL/dv for R = rotation_of_unit(v)"""
    r, x, y, z = v.unbind(-1)
    g = lambda b, a: G[..., b, a]
    return 2 * torch.stack([
        -z * g(0, 1) + y * g(0, 2) + z * g(1, 0) - x * g(1, 2) - y * g(2, 0) + x * g(2, 1),
        y * g(0, 1) + z * g(0, 2) + y * g(1, 0) - 2 * x * g(1, 1) - r * g(1, 2) + z * g(2, 0) + r * g(2, 1) - 2 * x * g(2, 2),
        -2 * y * g(0, 0) + x * g(0, 1) + r * g(0, 2) + x * g(1, 0) + z * g(1, 2) - r * g(2, 0) + z * g(2, 1) - 2 * y * g(2, 2),
        -2 * z * g(0, 0) - r * g(0, 1) + x * g(0, 2) + r * g(1, 0) - 2 * z * g(1, 1) + y * g(1, 2) + x * g(2, 0) + y * g(2, 1)], dim=-1)


def analytic_grads(xyz, rotation, t, lambdas=LAMBDAS):
    """-> (grad_xyz (P, 3), grad_rot (P, 4), S_xyz (P,), S_rot (P,)) float64"""
    dt = torch.float64
    j, valid, o, d, w, p = _tables(t, dt)
    x, r = xyz.detach().to(dt), rotation.detach().to(dt)
    P, K = j.shape
    ne = int(valid.sum())
    a_r, a_o, a_i = [lam / ne if ne else 0.0 for lam in lambdas]
    n = torch.sqrt((r * r).sum(-1, keepdim=True))
    q = r / n
    rel = quat_mult(q, p)
    nr = torch.sqrt((rel * rel).sum(-1, keepdim=True))
    v = rel / nr
    R = rotation_of_unit(v)
    c = x[j] - x[:, None]
    vm = valid.to(dt)
    u = torch.einsum("pba,pkb->pka", R, c) - o
    gu = (a_r * w * vm / torch.sqrt(w * (u * u).sum(-1) + EPS))[..., None] * u
    m = rel[j] - rel[:, None]
    gm = (a_o * w * vm / torch.sqrt(w * (m * m).sum(-1) + EPS))[..., None] * m           # into rel_j; -gm into rel_i
    mag = torch.sqrt((c * c).sum(-1) + EPS)
    gl = a_i * w * vm * (mag - d) / torch.sqrt(w * (mag - d) ** 2 + EPS)
    gc = torch.einsum("pba,pka->pkb", R, gu) + (gl / mag)[..., None] * c                 # into x_j; -gc into x_i
    gv = _fold(torch.einsum("pkb,pka->pkba", c, gu), v[:, None])
    g_rigid = (gv - v[:, None] * (v[:, None] * gv).sum(-1, keepdim=True)) / nr[:, None]  # into rel_i, through build_rotation

    def chain(g, rows):   # dL/drel of the rows -> dL/d(raw rotation): the product with p, then the normalisation
        gq = quat_mult(g, quat_conj(p[rows]))
        return (gq - q[rows] * (q[rows] * gq).sum(-1, keepdim=True)) / n[rows]

    own = torch.arange(P)[:, None].expand(P, K)
    centre_rot = [chain(g_rigid, own), chain(-gm, own)]
    into = j[valid]                                                                      # ascending edge id
    in_rot = chain(gm[valid], into)
    grad_xyz = (-gc).sum(1).index_add_(0, into, gc[valid])
    grad_rot = (centre_rot[0] + centre_rot[1]).sum(1).index_add_(0, into, in_rot)
    S_xyz = gc.norm(dim=-1).sum(1).index_add_(0, into, gc[valid].norm(dim=-1))
    S_rot = (centre_rot[0].norm(dim=-1) + centre_rot[1].norm(dim=-1)).sum(1).index_add_(0, into, in_rot.norm(dim=-1))
    return grad_xyz, grad_rot, S_xyz, S_rot


def row_error(g, g64, S):
    """|g - g64| / S_j per row (Euclidean norm over the row), 0 where S_j is 0 and the row agrees exactly"""
    diff = (g.double() - g64).norm(dim=-1)
    return torch.where(S > 0, diff / S.clamp(min=1e-300), torch.where(diff == 0, torch.zeros_like(diff), torch.full_like(diff, float("inf"))))


def graph(idx, P):
    """the reverse adjacency of idx as tests/torch_knn.py builds it -> (offsets, edges) int32 tensors"""
    offsets, edges = torch_knn.graph(idx.numpy(), P)
    return torch.from_numpy(offsets), torch.from_numpy(edges)
