"""Fixed-budget training ("3D Gaussian Splatting as Markov Chain Monte Carlo"; gsplat's MCMCStrategy) as fused HIP kernels
(include/gsr_mcmc.h), on the optimiser's leaves as fused_params lays them out:

    inject_noise(xyz, opacity, scaling, rotation, scaler)      after every optimiser step: xyz += Sigma (eps * gate(opacity) * scaler)
    relocate(optimizer, dst, src)                              rows dst become copies of rows src; the opacity and scales of a source
                                                               and its copies are recomputed so that the rendered distribution is kept
    regularizer(opacity, scaling, opacity_reg, scale_reg)      opacity_reg * mean(sigmoid(opacity)) + scale_reg * mean(exp(scaling))
    relocate_dead(optimizer), add_new(optimizer, cap_max)      gsplat's bookkeeping around relocate: which rows, onto which

    loss = training_loss(image, gt) + regularizer(opacity, scaling)
    loss.backward(); optimizer.step()
    inject_noise(xyz, opacity, scaling, rotation, noise_lr * lr_xyz)
    if step % 100 == 0: relocate_dead(optimizer); add_new(optimizer, cap_max)

When the helpers are called and with which threshold stays with the training loop.  One launch for the noise, three for a relocation,
no floating-point atomics: every result is bitwise reproducible.  HIP tensors only (no CPU fallback).
"""
import ctypes
import math

import torch

from diff_gaussian_rasterization import _binding
from diff_gaussian_rasterization._binding import ptr

MAX_GROUPS = 8               # include/gsr.h GSR_ADAM_MAX_GROUPS
MAX_RATIO = 51               # include/gsr_mcmc.h GSR_MCMC_MAX_RATIO
REG_THREADS = 256            # GSR_MCMC_REG_THREADS
REG_ELEMS_PER_THREAD = 12    # GSR_MCMC_REG_ELEMS_PER_THREAD
# the optimiser groups that hold one row per Gaussian, by the names the reference gives them (gaussian_model.py:243-252)
LEAF_NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


class McmcGroup(ctypes.Structure):      # include/gsr_mcmc.h gsr_mcmc_group
    _fields_ = [("param", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p), ("row", ctypes.c_int32)]


class RelocateArgs(ctypes.Structure):   # include/gsr_mcmc.h gsr_mcmc_relocate_args
    _fields_ = [("P", ctypes.c_int), ("D", ctypes.c_int), ("ngroups", ctypes.c_int), ("opacity_group", ctypes.c_int),
                ("scale_group", ctypes.c_int), ("zero_src_moments", ctypes.c_int), ("min_opacity", ctypes.c_float),
                ("groups", ctypes.POINTER(McmcGroup)), ("dst", ctypes.c_void_p), ("src", ctypes.c_void_p), ("counts", ctypes.c_void_p),
                ("stream", ctypes.c_void_p)]


_i, _f, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
_lib, _run = _binding.declare("gsr_mcmc.h", {
    "gsr_mcmc_noise": (_i, [_i] + [_vp] * 5 + [_f, _vp]),
    "gsr_mcmc_relocate": (_i, [ctypes.POINTER(RelocateArgs)]),
    "gsr_mcmc_regularizer_scratch_bytes": (ctypes.c_size_t, [_i]),
    "gsr_mcmc_regularizer": (_i, [_i, _vp, _vp, _f, _f] + [_vp] * 5),
}, {"gsr_mcmc_group": McmcGroup, "gsr_mcmc_relocate_args": RelocateArgs})
_COLS = {"xyz": 3, "opacity": 1, "scaling": 3, "rotation": 4, "noise": 3}


def _check_leaves(xyz=None, opacity=None, scaling=None, rotation=None, noise=None):
    """Every refusal of the leaf tensors a call names, before the kernel library is touched.  -> P"""
    named = [(n, t) for n, t in (("xyz", xyz), ("opacity", opacity), ("scaling", scaling), ("rotation", rotation), ("noise", noise))
             if t is not None]
    P = _binding.check_rows(named, _COLS)
    dev = named[0][1].device
    if dev.type != "cuda" or any(t.device != dev for _, t in named):
        raise RuntimeError("the leaves must be HIP (cuda) tensors on one device; the MCMC kernels have no CPU path")
    return P


@torch.no_grad()
def inject_noise(xyz, opacity, scaling, rotation, scaler, noise=None, generator=None):
    """gsplat's inject_noise_to_position, in place on xyz (P,3): xyz += Sigma (noise * gate * scaler) with Sigma = R diag(exp(scaling))^2 R^T
    of the normalised `rotation` (P,4), gate = 1 / (1 + exp(-100 ((1 - sigmoid(opacity)) - 0.995))) and scaler = noise_lr * lr_xyz.
    noise (P,3): the standard-normal draw; drawn here with torch.randn(generator=) where it is not given.  -> xyz"""
    P = _check_leaves(xyz, opacity, scaling, rotation, noise)
    if not xyz.is_contiguous():
        raise RuntimeError("xyz is changed in place and must be contiguous")
    dev = xyz.device
    with torch.cuda.device(dev):
        if noise is None:
            noise = torch.randn((P, 3), dtype=torch.float32, device=dev, generator=generator)
        o, s, q, n = (t.detach().contiguous() for t in (opacity, scaling, rotation, noise))
        _run("gsr_mcmc_noise", P, xyz.data_ptr(), o.data_ptr(), s.data_ptr(), q.data_ptr(), n.data_ptr(), float(scaler),
             torch.cuda.current_stream(dev).cuda_stream)
    return xyz


def _leaf_groups(optimizer, need=("opacity", "scaling"), needs="one param group named 'opacity' and one named 'scaling'"):
    """The param groups of an optimiser that hold one row per Gaussian, by their `name` -> [(name, group)].  need: the names that must
    be among them; needs: how the refusal words that (fused_densify asks for at least one group, whichever)."""
    found = [(g.get("name"), g) for g in optimizer.param_groups if g.get("name") in LEAF_NAMES]
    names = [n for n, _ in found]
    if not found or any(n not in names for n in need) or len(set(names)) != len(names):
        raise RuntimeError(f"the optimizer needs {needs} (the names taken: {LEAF_NAMES}); "
                           f"got {[g.get('name') for g in optimizer.param_groups]}")
    for n, g in found:
        if len(g["params"]) != 1:
            raise RuntimeError(f"group {n!r}: one tensor per group, as the reference builds its optimiser; got {len(g['params'])}")
    return found


def _optimizer_rows(optimizer, found):
    """The groups _leaf_groups found -> ([(param, exp_avg or None, exp_avg_sq or None)], their names)"""
    rows = []
    for _, g in found:
        p = g["params"][0]
        st = optimizer.state.get(p, {})
        rows.append((p, st.get("exp_avg"), st.get("exp_avg_sq")))
    return rows, [n for n, _ in found]


def _rows(groups, opacity_index, scaling_index):
    """groups -> ([(param, exp_avg or None, exp_avg_sq or None)], opacity index, scaling index)"""
    if isinstance(groups, torch.optim.Optimizer):
        rows, names = _optimizer_rows(groups, _leaf_groups(groups))
        return rows, names.index("opacity"), names.index("scaling")
    rows = [tuple(r) for r in groups]
    if any(len(r) != 3 for r in rows):
        raise RuntimeError("groups must be an optimizer or a list of (param, exp_avg, exp_avg_sq)")
    return rows, int(opacity_index), int(scaling_index)


def _check_relocate(groups, dst, src, min_opacity, opacity_index, scaling_index):
    """Every refusal of relocate() that needs no device work, before the kernel library is touched.  -> (rows, io, is, P, D)"""
    rows, io, isc = _rows(groups, opacity_index, scaling_index)
    if not 1 <= len(rows) <= MAX_GROUPS:
        raise RuntimeError(f"relocate takes 1..{MAX_GROUPS} groups; got {len(rows)}")
    if not (0 <= io < len(rows) and 0 <= isc < len(rows)) or io == isc:
        raise RuntimeError(f"opacity_index {io} and scaling_index {isc} must name two of the {len(rows)} groups")
    for k, (p, m, v) in enumerate(rows):
        if not torch.is_tensor(p) or not all(t is None or torch.is_tensor(t) for t in (m, v)):
            raise TypeError(f"group {k}: param, exp_avg and exp_avg_sq must be tensors (the moments may be None)")
    P = int(rows[io][0].shape[0]) if rows[io][0].dim() else 0
    dev = rows[io][0].device
    if dev.type != "cuda":
        raise RuntimeError("the groups must be HIP (cuda) tensors on one device; the MCMC kernels have no CPU path")
    if P < 1 or tuple(rows[io][0].shape) != (P, 1) or tuple(rows[isc][0].shape) != (P, 3):
        raise RuntimeError(f"the opacity group must be (P, 1) and the scaling group (P, 3) with P >= 1; got {tuple(rows[io][0].shape)}, "
                           f"{tuple(rows[isc][0].shape)}")
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
                raise RuntimeError(f"group {k}: {n} is changed in place and must be contiguous")
    for n, t in (("dst", dst), ("src", src)):
        if not torch.is_tensor(t):
            raise TypeError(f"{n} must be a tensor")
        if t.dim() != 1 or t.dtype != torch.int64:
            raise RuntimeError(f"{n} must be a 1-D int64 tensor (what torch.nonzero and torch.multinomial return); got {t.dtype} {tuple(t.shape)}")
        if t.device != dev:
            raise RuntimeError(f"{n} is on {t.device}, the groups on {dev}")
    if dst.shape != src.shape:
        raise RuntimeError(f"dst and src must have one length; got {tuple(dst.shape)}, {tuple(src.shape)}")
    if not 0.0 < float(min_opacity) < 1.0:
        raise ValueError(f"min_opacity must lie in (0, 1); got {min_opacity}")
    return rows, io, isc, P, int(dst.numel())


@torch.no_grad()
def relocate(groups, dst, src, min_opacity=0.005, zero_src_moments=True, check=True, opacity_index=3, scaling_index=4):
    """gsplat's relocate / sample_add without the sampling: for every j, row dst[j] of every group becomes a copy of row src[j], and
    the opacity logit and the log-scales of the source and of its copies are recomputed (compute_relocation, in double precision):
    with n = min(51, 1 + the number of times src[j] is named) and o the source's opacity, o' = 1 - (1 - o)^(1/n) clamped to
    [min_opacity, 1 - 2^-23] and scales * o / sum_{i<=n} sum_{k<i} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1).
    groups: a FusedAdam (or any optimizer of that state layout) -- its param groups named in LEAF_NAMES are taken, with the moments its
    state holds -- or a list of (param, exp_avg, exp_avg_sq), the moments None where there are none, in which opacity_index and
    scaling_index name the opacity (P,1) and the log-scale (P,3) entry (default: the order of fused_params' leaves).
    zero_src_moments: both moments of every source row become +0.0.  The moments of dst rows and state["step"] are never touched.
    dst, src: int64 (D,) on the groups' device; dst must hold no row twice and no row of src.  check=True verifies that (and the range
    of both) with torch operations, which wait for the device, and raises.
    Growing the set: enlarge the tensors, pass the new rows as dst and zero_src_moments=False (add_new does that)."""
    rows, io, isc, P, D = _check_relocate(groups, dst, src, min_opacity, opacity_index, scaling_index)
    if D == 0:
        return
    dev = rows[io][0].device
    with torch.cuda.device(dev):
        if check:
            both = torch.cat([dst, src])
            if bool(((both < 0) | (both >= P)).any()):
                raise RuntimeError(f"relocate: an index lies outside [0, {P})")
            if int(torch.unique(dst).numel()) != D:
                raise RuntimeError("relocate: dst names a row twice")
            if bool(torch.isin(dst, src).any()):
                raise RuntimeError("relocate: a row is both in dst and in src")
        d, s = dst.contiguous(), src.contiguous()
        table = (McmcGroup * len(rows))()
        for k, (p, m, v) in enumerate(rows):
            row = p.numel() // P
            table[k] = McmcGroup(p.data_ptr() if row else None, None if m is None or not row else m.data_ptr(),
                                 None if v is None or not row else v.data_ptr(), row)
        counts = torch.empty(P, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev)
        a = RelocateArgs(P=P, D=D, ngroups=len(rows), opacity_group=io, scale_group=isc, zero_src_moments=int(bool(zero_src_moments)),
                         min_opacity=float(min_opacity), groups=table, dst=d.data_ptr(), src=s.data_ptr(), counts=counts.data_ptr(),
                         stream=stream.cuda_stream)
        _run("gsr_mcmc_relocate", ctypes.byref(a))
        for t in (counts, d, s):
            t.record_stream(stream)


def regularizer_and_grads(opacity, scaling, opacity_reg=0.01, scale_reg=0.01, want=("opacity", "scaling")):
    """-> (value (1,) device tensor, {"opacity": d/dopacity (P,1), "scaling": d/dscaling (P,3)}), raw and without autograd; the
    dictionary holds the gradients named in `want`, formed in the same pass as the value."""
    P = _check_leaves(opacity=opacity, scaling=scaling)
    for k in want:
        if k not in ("opacity", "scaling"):
            raise ValueError(f"want: unknown gradient {k!r}; the choices are ('opacity', 'scaling')")
    lib = _lib()
    dev = opacity.device
    o, s = opacity.detach().contiguous(), scaling.detach().contiguous()
    with torch.cuda.device(dev):
        val = torch.empty(1, dtype=torch.float32, device=dev)
        grads = {k: torch.empty_like(t) for k, t in (("opacity", o), ("scaling", s)) if k in want}
        scratch = torch.empty(lib.gsr_mcmc_regularizer_scratch_bytes(P), dtype=torch.uint8, device=dev)
        _run("gsr_mcmc_regularizer", P, o.data_ptr(), s.data_ptr(), float(opacity_reg), float(scale_reg), val.data_ptr(),
             ptr(grads.get("opacity")), ptr(grads.get("scaling")), scratch.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        scratch.record_stream(torch.cuda.current_stream(dev))
    return val, grads


class _Regularizer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opacity, scaling, opacity_reg, scale_reg):
        want = tuple(n for n, need in zip(("opacity", "scaling"), ctx.needs_input_grad) if need)   # and no other gradient is computed
        val, grads = regularizer_and_grads(opacity, scaling, opacity_reg, scale_reg, want)
        ctx.want = want
        ctx.save_for_backward(*(grads[n] for n in want))
        return val[0]

    @staticmethod
    def backward(ctx, g_val):
        grads = dict(zip(ctx.want, ctx.saved_tensors))
        return tuple(grads[n] * g_val if n in grads else None for n in ("opacity", "scaling")) + (None, None)


def regularizer(opacity, scaling, opacity_reg=0.01, scale_reg=0.01):
    """gsplat's MCMC regulariser on the leaves: opacity_reg * mean(sigmoid(opacity)) + scale_reg * mean(exp(scaling)), a scalar tensor,
    differentiable w.r.t. both; value and gradients come from one pass over the leaves."""
    _check_leaves(opacity=opacity, scaling=scaling)
    return _Regularizer.apply(opacity, scaling, float(opacity_reg), float(scale_reg))


def _opacities(optimizer):
    found = dict(_leaf_groups(optimizer))
    logits = found["opacity"]["params"][0]
    _check_leaves(opacity=logits)
    return torch.sigmoid(logits.detach()).flatten()


@torch.no_grad()
def relocate_dead(optimizer, min_opacity=0.005, generator=None):
    """gsplat's relocate: every dead row (opacity <= min_opacity) moves onto a live row drawn with torch.multinomial in proportion to
    its opacity (generator: a generator of the parameters' device), the sources' moments are zeroed.  -> the number of rows moved."""
    opac = _opacities(optimizer)
    with torch.cuda.device(opac.device):
        dead = opac <= min_opacity
        dst = dead.nonzero(as_tuple=True)[0]
        D = int(dst.numel())
        if D == 0:
            return 0
        if D == int(opac.numel()):
            raise RuntimeError("relocate_dead: no Gaussian is alive")
        src = torch.multinomial(torch.where(dead, torch.zeros_like(opac), opac), D, replacement=True, generator=generator)
        relocate(optimizer, dst, src, min_opacity=min_opacity, zero_src_moments=True, check=False)
    return D


@torch.no_grad()
def add_new(optimizer, cap_max, factor=1.05, generator=None, min_opacity=0.005):
    """gsplat's sample_add: the set grows to min(cap_max, ceil(factor * P)) rows.  Every leaf group of the optimizer gets a new, longer
    parameter (its state moves with it, the new rows' moments are zero, `step` stays) -- fetch the parameters from
    optimizer.param_groups afterwards -- and the new rows are copies of rows drawn in proportion to their opacity, rescaled together
    with their sources; no moment is zeroed.  -> the number of rows added."""
    opac = _opacities(optimizer)
    P = int(opac.numel())
    n = max(0, min(int(cap_max), math.ceil(factor * P)) - P)
    if n == 0:
        return 0
    dev = opac.device
    with torch.cuda.device(dev):
        src = torch.multinomial(opac, n, replacement=True, generator=generator)
        for _, group in _leaf_groups(optimizer):
            old = group["params"][0]
            grown = torch.nn.Parameter(torch.cat([old.detach(), old.new_zeros((n,) + tuple(old.shape[1:]))]), requires_grad=old.requires_grad)
            state = optimizer.state.pop(old, None)
            if state is not None:
                for key in ("exp_avg", "exp_avg_sq"):
                    if key in state:
                        state[key] = torch.cat([state[key], state[key].new_zeros((n,) + tuple(old.shape[1:]))])
                optimizer.state[grown] = state
            group["params"][0] = grown
        relocate(optimizer, torch.arange(P, P + n, dtype=torch.int64, device=dev), src, min_opacity=min_opacity, zero_src_moments=False,
                 check=False)
    return n
