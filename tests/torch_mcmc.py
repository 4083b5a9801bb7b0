"""The three formulas of fixed-budget (MCMC) training (include/gsr_mcmc.h, fused_mcmc.py) written out in torch: the float64 reference
of tests/test_mcmc_cpu.py and tests/test_mcmc_gpu.py, the stock float32 sequence the noise bar is scaled by, and the inputs those
tests share.

    noise:      o = sigmoid(l), s = exp(ls), R = R(q / |q|), Sigma = R diag(s^2) R^T, gate = 1 / (1 + exp(-100 ((1 - o) - 0.995))),
                displacement = Sigma (eps gate scaler)
    relocation: n = min(51, 1 + times the source is named), o' = 1 - (1 - o)^(1/n),
                denom = sum_{i=1..n} sum_{k=0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1),
                new logit = logit(clamp(o', min_opacity, 1 - 2^-23)), new log-scales = log((o / denom) s)
    regulariser: w_o mean(sigmoid(l)) + w_s mean(exp(ls)), d/dl = (w_o / P) sigmoid(l) sigmoid(-l), d/dls = (w_s / (3 P)) exp(ls)
"""
import math

import torch

MAX_RATIO = 51
GATE_K, GATE_X0 = 100.0, 0.995
OPACITY_MAX = 1.0 - 2.0 ** -23


def rotation_matrices(q):
    """(P,4) unit quaternions (r, x, y, z) -> (P,3,3), the matrix the kernels build (csrc/gsr_device.h gsr_build_R)"""
    r, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)


def gate(opacity_logits):
    o = torch.sigmoid(opacity_logits.reshape(-1))
    return 1.0 / (1.0 + torch.exp(-GATE_K * ((1.0 - o) - GATE_X0)))


def noise_displacement(opacity, scaling, rotation, noise, scaler, dtype=torch.float64):
    """-> (displacement (P,3), gate (P,), ||Sigma||_F (P,)) in dtype"""
    l, ls, q, eps = (t.to(dtype) for t in (opacity, scaling, rotation, noise))
    R = rotation_matrices(q / q.norm(dim=-1, keepdim=True))
    sigma = R @ torch.diag_embed(torch.exp(ls) ** 2) @ R.transpose(1, 2)
    g = gate(l)
    return (sigma @ (eps * g[:, None] * scaler)[..., None])[..., 0], g, sigma.flatten(1).norm(dim=1)


def stock_noise_displacement(opacity, scaling, rotation, noise, scaler, dtype=torch.float32):
    """The sequence a user writes in stock PyTorch (gsplat's inject_noise_to_position with quat_scale_to_covar), in dtype:
    normalise, R, M = R S, Sigma = bmm(M, M^T), sigmoid, the gate, an einsum -> displacement (P,3)"""
    l, ls, q, eps = (t.to(dtype) for t in (opacity, scaling, rotation, noise))
    R = rotation_matrices(torch.nn.functional.normalize(q, dim=-1))
    M = R * torch.exp(ls)[:, None, :]
    covars = torch.bmm(M, M.transpose(1, 2))
    opacities = torch.sigmoid(l).flatten()
    op_sigmoid = 1 / (1 + torch.exp(-GATE_K * ((1 - opacities) - GATE_X0)))
    return torch.einsum("bij,bj->bi", covars, eps * op_sigmoid.unsqueeze(-1) * scaler)


def normalised_noise_error(got, ref, g, fro, noise, scaler):
    """per Gaussian: ||got - ref|| / (||Sigma||_F ||eps|| gate scaler), all in float64"""
    return (got.double() - ref).norm(dim=1) / (fro * noise.double().norm(dim=1) * g * scaler)


def relocation_denominator(o_new, n):
    """the double loop of gsplat's compute_relocation for one source, in Python floats (float64)"""
    denom = 0.0
    for i in range(1, n + 1):
        for k in range(i):
            denom += math.comb(i - 1, k) * (-1) ** k * o_new ** (k + 1) / math.sqrt(k + 1)
    return denom


def collapsed_denominator(o_new, n):
    """the same by the hockey-stick identity sum_{i=k+1..n} C(i-1, k) = C(n, k+1)"""
    return sum(math.comb(n, k + 1) * (-1) ** k * o_new ** (k + 1) / math.sqrt(k + 1) for k in range(n))


def relocation_values(logit, log_scales, n, min_opacity):
    """one source: logit (float), log_scales (3 floats), n -> (new logit, [new log-scales]) in float64"""
    l = torch.tensor(float(logit), dtype=torch.float64)
    o, q = float(torch.sigmoid(l)), float(torch.sigmoid(-l))   # q = 1 - o, without the subtraction
    o_new = 1.0 - q ** (1.0 / n)
    ratio = o / relocation_denominator(o_new, n)
    oc = min(max(o_new, min_opacity), OPACITY_MAX)
    return math.log(oc / (1.0 - oc)), [math.log(ratio * math.exp(float(v))) for v in log_scales]


def relocate(params, moments, dst, src, opacity_index, scaling_index, min_opacity=0.005, zero_src_moments=True):
    """params: [float32 (P, ...)]; moments: [(exp_avg, exp_avg_sq) or None] -> (new params, new moments, {row: (logit64, [ls64])}):
    what the call must leave behind, the two recomputed groups rounded once from float64."""
    P = params[0].shape[0]
    params = [p.clone() for p in params]
    moments = [None if m is None else (m[0].clone(), m[1].clone()) for m in moments]
    old = [p.clone() for p in params]
    counts = torch.bincount(src, minlength=P)
    exact = {}
    for d, s in zip(dst.tolist(), src.tolist()):
        n = min(MAX_RATIO, int(counts[s]) + 1)
        if s not in exact:
            exact[s] = relocation_values(old[opacity_index][s, 0], old[scaling_index][s], n, min_opacity)
        exact[d] = exact[s]
        for k, p in enumerate(params):
            if k == opacity_index:
                p[d, 0] = p[s, 0] = torch.tensor(exact[s][0], dtype=torch.float64).float()
            elif k == scaling_index:
                p[d] = p[s] = torch.tensor(exact[s][1], dtype=torch.float64).float()
            else:
                p[d] = old[k][s]
            if zero_src_moments and moments[k] is not None:
                moments[k][0][s] = 0.0
                moments[k][1][s] = 0.0
    return params, moments, exact


def regularizer(opacity, scaling, w_o, w_s):
    """-> (value, d/dopacity (P,1), d/dscaling (P,3)) in float64"""
    l, ls = opacity.double(), scaling.double()
    P = l.shape[0]
    val = w_o * torch.sigmoid(l).mean() + w_s * torch.exp(ls).mean()
    return val, (w_o / P) * torch.sigmoid(l) * torch.sigmoid(-l), (w_s / (3 * P)) * torch.exp(ls)


def make_leaves(P, rest=15, seed=0, logit_range=9.0):
    """the six leaves in fused_params' order: xyz (P,3), features_dc (P,1,3), features_rest (P,rest,3), opacity logits (P,1) uniform in
    [-logit_range, logit_range], log-scales (P,3) uniform in [-6, 2], quaternions (P,4) with norms uniform in [0.1, 10]; float32.
    No coordinate of xyz is closer to zero than 1e-3."""
    g = torch.Generator().manual_seed(1000 + seed)
    xyz = 3.0 * torch.randn(P, 3, generator=g)
    xyz = torch.where(xyz.abs() < 1e-3, torch.full_like(xyz, 1e-3), xyz)
    dc = torch.randn(P, 1, 3, generator=g)
    fr = torch.randn(P, rest, 3, generator=g)
    opacity = (2 * torch.rand(P, 1, generator=g) - 1) * logit_range
    scaling = -6.0 + 8.0 * torch.rand(P, 3, generator=g)
    q = torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=-1) * (0.1 + 9.9 * torch.rand(P, 1, generator=g))
    return [xyz, dc, fr, opacity, scaling, q]
