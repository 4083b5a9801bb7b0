"""Densification (include/gsr_densify.h, fused_densify.py) written out in torch: the float64 reference of tests/test_densify_cpu.py and
tests/test_densify_gpu.py, the stock sequence a user of the reference writes, and the inputs those tests share.

    (a) expand(leaves, moments, action, noise): the contract.  Output rows: survivors (KEEP, CLONE) in index order, clone copies in source
        order, first children of the split rows in source order, second children.  Survivors carry parameter and moments; new rows carry
        the parameter and zero moments; child k of the j-th split row (source i) takes n = noise[k S + j]:
        xyz_i + R(q_i / |q_i|) (exp(ls_i) * n) in float64, log-scales fp32(float64(ls_i) - log 1.6).
    (b) stock_densify_and_prune(...): GaussianModel.densify_and_prune of the reference (scene/gaussian_model.py:565-594) as its sequence
        of boolean masks and torch.cat on every parameter and both moments -- densify_and_clone (:543-563), densify_and_split (:500-541)
        with cat_tensors_to_optimizer (:447-471) and densification_postfix (:473-498), then prune_points (:421-445) with _prune_optimizer
        (:394-419) -- with the normal draw handed in: torch.normal(0, stds) is stds * noise.
"""
import math

import torch

import torch_mcmc

KEEP, PRUNE, CLONE, SPLIT = 0, 1, 2, 3
LOG_SHRINK = 0.47000362924573558   # include/gsr_densify.h GSR_DENSIFY_LOG_SHRINK
MAX_GRAD, MIN_OPACITY, EXTENT, PERCENT_DENSE, SCREEN = 2e-4, 0.005, 20.0, 0.01, 20
XYZ, OPACITY, SCALING, ROTATION = 0, 3, 4, 5   # positions in make_leaves' list


def source_rows(action):
    """action (P,) -> (the source row of every output row (P',) int64, K, C, S)"""
    a = action.to(torch.int64)
    idx = torch.arange(a.numel())
    keep, clone, split = idx[(a == KEEP) | (a == CLONE)], idx[a == CLONE], idx[a == SPLIT]
    return torch.cat([keep, clone, split, split]), int(keep.numel()), int(clone.numel()), int(split.numel())


def child_displacement(scaling, rotation, noise, dtype=torch.float64):
    """rows of the split sources, (S,3) and (S,4), and noise (2S,3) -> (R(q/|q|) (exp(ls) * n) (2S,3), ||exp(ls) * n|| (2S,)) in dtype"""
    ls, q, n = scaling.to(dtype).repeat(2, 1), rotation.to(dtype).repeat(2, 1), noise.to(dtype)
    t = torch.exp(ls) * n
    R = torch_mcmc.rotation_matrices(q / q.norm(dim=-1, keepdim=True))
    return (R @ t[..., None])[..., 0], t.norm(dim=1)


def stock_child_displacement(scaling, rotation, noise, dtype=torch.float32):
    """the same as the reference forms it (:523-529): stds repeated, samples = stds * noise, build_rotation of the unnormalised
    quaternion (utils/general_utils.py: q / sqrt(sum q^2), then the nine entries), a bmm"""
    ls, q, n = scaling.to(dtype), rotation.to(dtype), noise.to(dtype)
    stds = torch.exp(ls).repeat(2, 1)
    samples = stds * n
    norm = torch.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    rots = torch_mcmc.rotation_matrices(q / norm[:, None]).repeat(2, 1, 1)
    return torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1)


def expand(leaves, moments, action, noise=None, extras=()):
    """leaves: make_leaves' list (float32); moments: [(exp_avg, exp_avg_sq) or None]; action (P,) uint8; noise (2S,3); extras:
    [(tensor, zero_new)] -> dict: leaves (float32; children's xyz rounded once from float64), moments, extras, src, counts (K, C, S),
    xyz64 (the children's positions (2S,3) in float64), d64 (their displacements), scale (||exp(ls) * n||)"""
    src, K, C, S = source_rows(action)
    out = [t[src].clone() for t in leaves]
    d64 = torch.zeros(0, 3, dtype=torch.float64)
    scale = torch.zeros(0, dtype=torch.float64)
    xyz64 = d64
    if S:
        split = src[K + C:K + C + S]
        d64, scale = child_displacement(leaves[SCALING][split], leaves[ROTATION][split], noise)
        xyz64 = leaves[XYZ][split].double().repeat(2, 1) + d64
        out[XYZ][K + C:] = xyz64.float()
        out[SCALING][K + C:] = (leaves[SCALING][split].double().repeat(2, 1) - LOG_SHRINK).float()
    new_moments = []
    for m in moments:
        if m is None:
            new_moments.append(None)
            continue
        pair = []
        for t in m:
            o = t[src].clone()
            o[K:] = 0.0
            pair.append(o)
        new_moments.append(tuple(pair))
    new_extras = []
    for t, zero_new in extras:
        o = t[src].clone()
        if zero_new:
            o[K:] = 0
        new_extras.append(o)
    return dict(leaves=out, moments=new_moments, extras=new_extras, src=src, counts=(K, C, S), xyz64=xyz64, d64=d64, scale=scale)


def stock_densify_and_prune(leaves, moments, grads, max_grad, min_opacity, extent, max_screen_size, noise, percent_dense=PERCENT_DENSE):
    """-> (leaves, [(exp_avg, exp_avg_sq)]) after the reference's clone, split, prune; float32 as the reference runs it"""
    params = [t.clone() for t in leaves]
    moments = [(m.clone(), v.clone()) for m, v in moments]
    P = params[0].shape[0]

    def append(new):        # cat_tensors_to_optimizer (:447-471): the new rows behind the old ones, zero moments for them
        for k, t in enumerate(new):
            params[k] = torch.cat((params[k], t), dim=0)
            moments[k] = tuple(torch.cat((s, torch.zeros_like(t)), dim=0) for s in moments[k])

    def keep(mask):         # _prune_optimizer (:394-419)
        for k in range(len(params)):
            params[k] = params[k][mask]
            moments[k] = tuple(s[mask] for s in moments[k])

    grads = grads.clone().reshape(P, 1)
    grads[grads.isnan()] = 0.0                                                              # :575-576
    sel = torch.norm(grads, dim=-1) >= max_grad                                             # densify_and_clone, :550-552
    sel = sel & (torch.exp(params[SCALING]).max(dim=1).values <= percent_dense * extent)
    append([t[sel] for t in params])
    n_init = params[0].shape[0]                                                             # densify_and_split, :513-520
    padded = torch.zeros(n_init)
    padded[:P] = grads.squeeze(-1)
    sel = (padded >= max_grad) & (torch.exp(params[SCALING]).max(dim=1).values > percent_dense * extent)
    new = [t[sel].repeat(*([2] + [1] * (t.dim() - 1))) for t in params]                     # :532-535
    new[XYZ] = stock_child_displacement(params[SCALING][sel], params[ROTATION][sel], noise) + params[XYZ][sel].repeat(2, 1)   # :523-529
    new[SCALING] = torch.log(torch.exp(params[SCALING][sel]).repeat(2, 1) / (0.8 * 2))      # :531
    append(new)
    keep(~torch.cat((sel, torch.zeros(2 * int(sel.sum()), dtype=torch.bool))))              # :540-541
    max_radii2D = torch.zeros(params[0].shape[0])                                           # densification_postfix, :498
    prune = (torch.sigmoid(params[OPACITY]) < min_opacity).squeeze(-1)                      # :587-591
    if max_screen_size:
        big_vs = max_radii2D > max_screen_size
        big_ws = torch.exp(params[SCALING]).max(dim=1).values > 0.1 * extent
        prune = prune | big_vs | big_ws
    keep(~prune)                                                                            # :594
    return params, moments


def make_case(P, rest=15, seed=0):
    """-> (leaves, moments, grads (P,1)): make_leaves' six tensors, random moments, and mean gradients uniform in [0, 2 MAX_GRAD] with a
    few NaN.  Every quantity a threshold is applied to is moved off it where it came closer than 2e-3 relative, so that a decision
    taken in float32 is the float64 one (margins() measures it)."""
    leaves = torch_mcmc.make_leaves(P, rest=rest, seed=seed)
    g = torch.Generator().manual_seed(5000 + seed)
    moments = [(torch.randn(t.shape, generator=g), torch.rand(t.shape, generator=g)) for t in leaves]
    grads = 2 * MAX_GRAD * torch.rand(P, 1, generator=g)
    grads = torch.where((grads / MAX_GRAD - 1).abs() < 2e-3, torch.full_like(grads, 1.01 * MAX_GRAD), grads)
    grads[torch.rand(P, 1, generator=g) < 0.03] = float("nan")
    ls = leaves[SCALING]
    for thr in (PERCENT_DENSE * EXTENT, 0.1 * EXTENT, 0.16 * EXTENT):
        ls[(ls - math.log(thr)).abs() < 2e-3] = math.log(thr) + 0.01
    l = leaves[OPACITY]
    l[(torch.sigmoid(l.double()) / MIN_OPACITY - 1).abs() < 2e-3] += 0.05
    return leaves, moments, grads


def margins(leaves, grads):
    """the smallest relative distance, in float64, of a tested quantity from its threshold -> float"""
    smax = torch.exp(leaves[SCALING].double()).max(dim=1).values
    g = torch.nan_to_num(grads.double().reshape(-1), nan=0.0).abs()
    rel = [(g / MAX_GRAD - 1).abs().min(), (torch.sigmoid(leaves[OPACITY].double()) / MIN_OPACITY - 1).abs().min()]
    rel += [(smax / thr - 1).abs().min() for thr in (PERCENT_DENSE * EXTENT, 0.1 * EXTENT, 0.16 * EXTENT)]
    return float(min(rel))
