"""The structural edit of adaptive density control (the reference's GaussianModel.densify_and_prune, scene/gaussian_model.py:394-594;
gsplat's DefaultStrategy) as one fused compaction (include/gsr_densify.h), on the optimiser's leaves as fused_params lays them out:

    densify(groups, action)                  one action code per row -- KEEP, PRUNE, CLONE, SPLIT -- and every parameter tensor, both of
                                             its moments and every extra tensor is written once into new storage
    prune(groups, mask)                      the reference's prune_points
    action_codes(opacity, scaling, grads, max_grad, min_opacity, extent, ...)
                                             the codes with which densify ends where the reference's densify_and_prune ends
    densify_and_prune(optimizer, stats, max_grad, min_opacity, extent, max_screen_size)
                                             the two together, with fresh zeroed densify_stats of the new size
    reset_opacity(optimizer)                 the reference's reset_opacity: logits capped at logit(0.01), their moments zeroed

    if step % 100 == 0:
        params, stats, _, _ = densify_and_prune(optimizer, stats, 0.0002, 0.005, extent, 20 if step > 3000 else None)
    if step % 3000 == 0: reset_opacity(optimizer)

When the helpers are called and with which thresholds stays with the training loop.  The output rows are the survivors in index order,
the clone copies in the order of their sources, the first child of every split row, the second child of every split row: the order the
reference's clone, split, prune sequence ends with.  Survivors keep their moments; new rows start with zero moments; state["step"] is
never touched.  No atomics: every result is bitwise reproducible.  HIP tensors only (no CPU fallback); action_codes and reset_opacity are
plain torch and run wherever their tensors are.
"""
import ctypes
import functools
import math

import torch

import fused_mcmc
from diff_gaussian_rasterization import _binding
from fused_mcmc import LEAF_NAMES

KEEP, PRUNE, CLONE, SPLIT = 0, 1, 2, 3     # include/gsr_densify.h GSR_DENSIFY_KEEP ..
SPLIT_N = 2                                # GSR_DENSIFY_SPLIT_N
MAX_GROUPS = 16                            # GSR_DENSIFY_MAX_GROUPS
PLAN_ROWS = 1024                           # GSR_DENSIFY_PLAN_ROWS
SCAN_THREADS = 256                         # GSR_DENSIFY_SCAN_THREADS
LOG_SHRINK = 0.47000362924573558           # GSR_DENSIFY_LOG_SHRINK, log(1.6)


class DensifyGroup(ctypes.Structure):      # include/gsr_densify.h gsr_densify_group
    _fields_ = [("param", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p), ("out_param", ctypes.c_void_p),
                ("out_exp_avg", ctypes.c_void_p), ("out_exp_avg_sq", ctypes.c_void_p), ("row", ctypes.c_int32), ("zero_new", ctypes.c_int32)]


class DensifyArgs(ctypes.Structure):       # include/gsr_densify.h gsr_densify_args
    _fields_ = [("P", ctypes.c_int), ("K", ctypes.c_int), ("C", ctypes.c_int), ("S", ctypes.c_int), ("ngroups", ctypes.c_int),
                ("xyz_group", ctypes.c_int), ("scale_group", ctypes.c_int), ("rotation_group", ctypes.c_int),
                ("groups", ctypes.POINTER(DensifyGroup)), ("action", ctypes.c_void_p), ("scratch", ctypes.c_void_p), ("noise", ctypes.c_void_p),
                ("src_of", ctypes.c_void_p), ("stream", ctypes.c_void_p)]


_lib, _run = _binding.declare("gsr_densify.h", {
    "gsr_densify_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "gsr_densify_plan": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 4),
    "gsr_densify_apply": (ctypes.c_int, [ctypes.POINTER(DensifyArgs)]),
}, {"gsr_densify_group": DensifyGroup, "gsr_densify_args": DensifyArgs})
bind = _binding.bind   # restype and argtypes on a library loaded by hand (tests load one beside the product's)
# the leaf groups as fused_mcmc finds them, but any of them will do: a densification names the ones it needs itself
_leaf_groups = functools.partial(fused_mcmc._leaf_groups, need=(), needs="param groups named as the reference names them, each once")


def _rows(groups, xyz_index, scaling_index, rotation_index):
    """groups -> ([(param, exp_avg or None, exp_avg_sq or None)], names or None, (xyz, scaling, rotation) indices, -1 for none)"""
    if isinstance(groups, torch.optim.Optimizer):
        rows, names = fused_mcmc._optimizer_rows(groups, _leaf_groups(groups))
        return rows, names, tuple(names.index(n) if n in names else -1 for n in ("xyz", "scaling", "rotation"))
    rows = [tuple(r) for r in groups]
    if not rows or any(len(r) != 3 for r in rows):
        raise RuntimeError("groups must be an optimizer or a non-empty list of (param, exp_avg, exp_avg_sq)")
    named = tuple(-1 if i is None or not 0 <= int(i) < len(rows) else int(i) for i in (xyz_index, scaling_index, rotation_index))
    return rows, None, named


def _check_densify(groups, action, noise, extras, xyz_index=0, scaling_index=4, rotation_index=5):
    """Every refusal of densify() that needs no device work, before the kernel library is touched.
    -> (rows, names, (xyz, scaling, rotation) indices, [(tensor, zero_new)], P)"""
    rows, names, named = _rows(groups, xyz_index, scaling_index, rotation_index)
    extras = [tuple(e) if isinstance(e, (tuple, list)) else (e,) for e in extras]
    if any(len(e) != 2 for e in extras):
        raise RuntimeError("extras must be a sequence of (tensor, zero_new) pairs")
    if len(rows) + len(extras) > MAX_GROUPS:
        raise RuntimeError(f"densify takes at most {MAX_GROUPS} groups, extras included; got {len(rows)} + {len(extras)}")
    for k, (p, m, v) in enumerate(rows):
        if not torch.is_tensor(p) or not all(t is None or torch.is_tensor(t) for t in (m, v)):
            raise TypeError(f"group {k}: param, exp_avg and exp_avg_sq must be tensors (the moments may be None)")
    for k, (t, _) in enumerate(extras):
        if not torch.is_tensor(t):
            raise TypeError(f"extra {k}: (tensor, zero_new) needs a tensor first")
    if not torch.is_tensor(action):
        raise TypeError("action must be a tensor")
    first = rows[0][0]
    P = int(first.shape[0]) if first.dim() else 0
    dev = first.device
    if dev.type != "cuda":
        raise RuntimeError("the groups must be HIP (cuda) tensors on one device; the densification kernels have no CPU path")
    if P < 1:
        raise RuntimeError(f"every group needs dim 0 = P >= 1; got {tuple(first.shape)}")
    for k, (p, m, v) in enumerate(rows):
        if p.dim() < 1 or p.shape[0] != P:
            raise RuntimeError(f"group {k}: every group needs dim 0 = P = {P}; got {tuple(p.shape)}")
        if (m is None) != (v is None):
            raise RuntimeError(f"group {k}: exp_avg and exp_avg_sq go together")
        for n, t in (("param", p), ("exp_avg", m), ("exp_avg_sq", v)):
            if t is None:
                continue
            if t.dtype != torch.float32 or t.device != dev or t.shape != p.shape:
                raise RuntimeError(f"group {k}: {n} must be float32, on {dev} and of shape {tuple(p.shape)}; got {t.dtype} {tuple(t.shape)} "
                                   f"on {t.device}")
            if not t.is_contiguous():
                raise RuntimeError(f"group {k}: {n} must be contiguous")
    for k, (t, _) in enumerate(extras):
        if t.dim() < 1 or t.shape[0] != P:
            raise RuntimeError(f"extra {k}: every extra needs dim 0 = P = {P}; got {tuple(t.shape)}")
        if t.dtype not in (torch.float32, torch.int32) or t.device != dev:
            raise RuntimeError(f"extra {k}: must be float32 or int32 (rows are copied as 32-bit words) and on {dev}; got {t.dtype} on {t.device}")
        if not t.is_contiguous():
            raise RuntimeError(f"extra {k}: must be contiguous")
    for i, (n, cols) in zip(named, (("xyz", 3), ("scaling", 3), ("rotation", 4))):
        if i >= 0 and tuple(rows[i][0].shape) != (P, cols):
            raise RuntimeError(f"the {n} group must be (P, {cols}); got {tuple(rows[i][0].shape)}")
    if len({i for i in named if i >= 0}) != sum(i >= 0 for i in named):
        raise RuntimeError(f"xyz, scaling and rotation must be three groups; got the indices {named}")
    if action.dtype != torch.uint8 or tuple(action.shape) != (P,):
        raise RuntimeError(f"action must be uint8 of shape ({P},), one code per row; got {action.dtype} {tuple(action.shape)}")
    if action.device != dev:
        raise RuntimeError(f"action is on {action.device}, the groups on {dev}")
    if noise is not None:
        if not torch.is_tensor(noise):
            raise TypeError("noise must be a tensor")
        if noise.dtype != torch.float32 or noise.dim() != 2 or noise.shape[1] != 3:
            raise RuntimeError(f"noise must be float32 of shape (2 S, 3), S the number of split rows; got {noise.dtype} {tuple(noise.shape)}")
        if noise.device != dev:
            raise RuntimeError(f"noise is on {noise.device}, the groups on {dev}")
    return rows, names, named, extras, P


@torch.no_grad()
def densify(groups, action, noise=None, generator=None, extras=(), xyz_index=0, scaling_index=4, rotation_index=5):
    """Clone, split and prune in one compaction.  action: uint8 (P,) on the groups' device, one code per row: KEEP (the row survives with
    its moments), PRUNE (no output row), CLONE (the row survives with its moments, plus one copy), SPLIT (the row is replaced by two
    children: xyz + R(q/|q|) (exp(scaling) * noise row), log-scales - log(1.6), everything else copied).  New rows have zero moments.
    groups: a FusedAdam (or any optimizer of that state layout) -- its param groups named in LEAF_NAMES are taken, with the moments its
    state holds, every one of them gets a new Parameter with its state moved over, and {name: new parameter} is returned: fetch the
    parameters from there or from optimizer.param_groups -- or a list of (param, exp_avg, exp_avg_sq), the moments None where there are
    none, in which xyz_index, scaling_index and rotation_index name the (P,3), (P,3) and (P,4) entries a split needs (default: the order
    of fused_params' leaves; an index that names no entry is fine while nothing is split), and a list of new (param, exp_avg,
    exp_avg_sq) is returned.
    noise: (2 S, 3) float32, the standard-normal draw of child k of the j-th split row in row k S + j; drawn here with
    torch.randn(generator=) where it is not given.  extras: (tensor, zero_new) pairs, float32 or int32 with dim 0 = P, that ride along
    (statistics, index tables); with zero_new their new rows are +0 instead of a copy.
    One read-back of four integers waits for the device.  A code above 3 raises and leaves everything as it was.
    -> (new parameters, [new extras], (K, C, S)): K rows kept, C of them cloned, S split; P' = K + C + 2 S."""
    rows, names, named, extras, P = _check_densify(groups, action, noise, extras, xyz_index, scaling_index, rotation_index)
    dev = rows[0][0].device
    with torch.cuda.device(dev):
        lib = _lib()
        stream = torch.cuda.current_stream(dev)
        act = action.contiguous()
        scratch = torch.empty(lib.gsr_densify_scratch_bytes(P), dtype=torch.uint8, device=dev)
        totals = torch.empty(4, dtype=torch.int32, device=dev)
        _run("gsr_densify_plan", P, act.data_ptr(), scratch.data_ptr(), totals.data_ptr(), stream.cuda_stream)
        K, C, S, bad = totals.tolist()   # the one read-back: P' must be known before the outputs can be allocated
        if bad:
            raise RuntimeError(f"densify: {bad} action codes lie above {SPLIT} (KEEP {KEEP}, PRUNE {PRUNE}, CLONE {CLONE}, SPLIT {SPLIT})")
        if S > 0:
            if min(named) < 0:
                raise RuntimeError("densify: a split needs the xyz, scaling and rotation groups")
            if noise is None:
                noise = torch.randn((SPLIT_N * S, 3), dtype=torch.float32, device=dev, generator=generator)
            elif noise.shape[0] != SPLIT_N * S:
                raise RuntimeError(f"noise must be ({SPLIT_N} S, 3) with S = {S} split rows; got {tuple(noise.shape)}")
            noise = noise.contiguous()
        Pout = K + C + SPLIT_N * S
        detached = [tuple(None if t is None else t.detach() for t in r) for r in rows]
        new = lambda t: None if t is None else torch.empty((Pout,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
        outs = [tuple(new(t) for t in r) for r in detached]
        extra_outs = [new(t) for t, _ in extras]
        table = (DensifyGroup * (len(rows) + len(extras)))()
        ptr = lambda t, row: None if t is None or not row else t.data_ptr()
        for k, ((p, m, v), (op, om, ov)) in enumerate(zip(detached, outs)):
            row = p.numel() // P
            table[k] = DensifyGroup(ptr(p, row), ptr(m, row), ptr(v, row), ptr(op, row), ptr(om, row), ptr(ov, row), row, 0)
        for k, ((t, zero_new), ot) in enumerate(zip(extras, extra_outs)):
            row = t.numel() // P
            table[len(rows) + k] = DensifyGroup(ptr(t, row), None, None, ptr(ot, row), None, None, row, int(bool(zero_new)))
        src_of = torch.empty(max(Pout, 1), dtype=torch.int32, device=dev)
        a = DensifyArgs(P=P, K=K, C=C, S=S, ngroups=len(table), xyz_group=named[0], scale_group=named[1], rotation_group=named[2],
                        groups=table, action=act.data_ptr(), scratch=scratch.data_ptr(), noise=None if S == 0 else noise.data_ptr(),
                        src_of=src_of.data_ptr(), stream=stream.cuda_stream)
        _run("gsr_densify_apply", ctypes.byref(a))
        for t in (act, scratch, src_of) + (() if S == 0 else (noise,)):
            t.record_stream(stream)
    if names is None:
        return outs, extra_outs, (K, C, S)
    fresh = {}
    for (name, group), (op, om, ov) in zip(_leaf_groups(groups), outs):
        old = group["params"][0]
        param = torch.nn.Parameter(op, requires_grad=old.requires_grad)
        state = groups.state.pop(old, None)
        if state is not None:
            if om is not None:
                state["exp_avg"], state["exp_avg_sq"] = om, ov
            groups.state[param] = state
        group["params"][0] = param
        fresh[name] = param
    return fresh, extra_outs, (K, C, S)


@torch.no_grad()
def prune(groups, mask, extras=()):
    """The reference's prune_points (scene/gaussian_model.py:421-445): the rows where `mask` (bool (P,)) is set leave every group, both
    moments and every extra; the rest keep their order and their moments.  -> as densify"""
    if not torch.is_tensor(mask) or mask.dtype != torch.bool or mask.dim() != 1:
        raise RuntimeError(f"mask must be a bool tensor of shape (P,); got {getattr(mask, 'dtype', type(mask))} {tuple(getattr(mask, 'shape', ()))}")
    return densify(groups, mask.to(torch.uint8) * PRUNE, extras=extras)


@torch.no_grad()
def action_codes(opacity, scaling, grads, max_grad, min_opacity, extent, max_screen_size=None, max_radii2D=None, percent_dense=0.01):
    """The codes with which densify ends with the set the reference's densify_and_prune (scene/gaussian_model.py:565-594) ends with;
    elementwise torch operations on (P,) tensors, on whichever device they are.  opacity (P,1) logits, scaling (P,3) log-scales, grads
    (P,) or (P,1): xyz_gradient_accum / denom.
        sel = |grads| >= max_grad (NaN counts as 0),  big = max exp(scaling) > percent_dense * extent
        CLONE where sel & ~big,  SPLIT where sel & big
    and the final prune test applied to what each row becomes: sigmoid(opacity) < min_opacity for originals, clones and children alike,
    and with max_screen_size set also max exp(scaling) > 0.1 * extent -- for children on the scale / 1.6.  A row whose outputs would
    all be pruned is PRUNE.  The reference zeroes max_radii2D in densification_postfix (:498) before it tests it (:589), so its
    screen-size test never fires and the default reproduces that; max_radii2D (P,) given explicitly applies max_radii2D > max_screen_size
    to the originals and to what comes of them, as gsplat's DefaultStrategy does.  -> uint8 (P,)"""
    P = opacity.shape[0]
    g = torch.nan_to_num(grads.detach().reshape(P), nan=0.0).abs()
    smax = torch.exp(scaling.detach()).max(dim=1).values
    low = torch.sigmoid(opacity.detach().reshape(P)) < min_opacity
    sel = g >= max_grad
    big = smax > percent_dense * extent
    codes = torch.where(sel & big, SPLIT, torch.where(sel, CLONE, KEEP))
    gone, child_gone = low, low
    if max_screen_size:
        gone, child_gone = low | (smax > 0.1 * extent), low | (smax / 1.6 > 0.1 * extent)
        if max_radii2D is not None:
            seen_big = max_radii2D.detach().reshape(P) > max_screen_size
            gone, child_gone = gone | seen_big, child_gone | seen_big
    return torch.where(torch.where(codes == SPLIT, child_gone, gone), PRUNE, codes).to(torch.uint8)


@torch.no_grad()
def densify_and_prune(optimizer, stats, max_grad, min_opacity, extent, max_screen_size, percent_dense=0.01, use_max_radii2D=False, noise=None,
                      generator=None, extras=()):
    """The reference's densify_and_prune on an optimiser whose groups are named in LEAF_NAMES: action_codes, then densify.
    stats: the densify_stats (xyz_gradient_accum, denom, max_radii2D) of GaussianRasterizer, (P,) or (P,1) each.  use_max_radii2D hands
    max_radii2D to action_codes, which the reference in effect never does (see there).
    -> ({name: new parameter}, fresh zeroed stats of P' rows, [new extras], (K, C, S))"""
    found = dict(_leaf_groups(optimizer))
    if "opacity" not in found or "scaling" not in found:
        raise RuntimeError(f"densify_and_prune needs the param groups 'opacity' and 'scaling'; got {list(found)}")
    if not isinstance(stats, (tuple, list)) or len(stats) != 3 or not all(torch.is_tensor(t) for t in stats):
        raise TypeError("stats must be the three tensors (xyz_gradient_accum, denom, max_radii2D)")
    accum, denom, radii = stats
    codes = action_codes(found["opacity"]["params"][0], found["scaling"]["params"][0], accum.reshape(-1) / denom.reshape(-1), max_grad, min_opacity,
                         extent, max_screen_size, radii if use_max_radii2D else None, percent_dense)
    params, new_extras, counts = densify(optimizer, codes, noise=noise, generator=generator, extras=extras)
    Pout = counts[0] + counts[1] + SPLIT_N * counts[2]
    fresh = tuple(torch.zeros((Pout,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in stats)
    return params, fresh, new_extras, counts


@torch.no_grad()
def reset_opacity(optimizer, max_opacity=0.01):
    """The reference's reset_opacity (scene/gaussian_model.py:310-321): logit <- min(logit, logit(max_opacity)) in place, and both moments
    of the opacity group zeroed.  Torch operations; no kernel.  -> the opacity parameter"""
    if not 0.0 < float(max_opacity) < 1.0:
        raise ValueError(f"max_opacity must lie in (0, 1); got {max_opacity}")
    found = dict(_leaf_groups(optimizer))
    if "opacity" not in found:
        raise RuntimeError(f"reset_opacity needs the param group 'opacity'; got {list(found)}")
    p = found["opacity"]["params"][0]
    p.data.clamp_(max=math.log(max_opacity / (1.0 - max_opacity)))
    state = optimizer.state.get(p, {})
    for key in ("exp_avg", "exp_avg_sq"):
        if key in state:
            state[key].zero_()
    return p
