"""4D Gaussians rendered at a time stamp ("Real-time Photorealistic Dynamic Scene Representation and Rendering with 4D Gaussian
Splatting", Yang et al.) as fused HIP kernels (include/gsr_slice4d.h), on the optimiser's leaves as fused_params lays them out and
named as the 4DGS model names them:

    slice_at(xyz, t, scaling, scaling_t, rotation, rotation_r, opacity, time, ...)   the 4D Gaussians conditioned on t = time ->
                                                         (means3D, cov3D, opacities[, velocity]): what the rasterizer takes as
                                                         means3D, cov3D_precomp and opacities; one launch forward, one backward
    harmonic_features(features_t, t, time, period)       SH coefficients modulated by a Fourier series in time - t -> shs
    visible_at(opacities)                                the mask 4DGS culls by

    out = render(camera, pc, pipe, bg, time=0.37)        # gaussian_renderer.render applies the three

Everything is evaluated in double from the float32 leaves and rounded once; the backward recomputes instead of saving.  No atomics:
every result is bitwise reproducible.  HIP tensors only (no CPU fallback).
"""
import ctypes
import functools
import math

import torch

from diff_gaussian_rasterization import _binding

THREADS = 256      # include/gsr_slice4d.h GSR_SLICE4D_THREADS
MAX_N = 3          # GSR_HARMONIC_MAX_N
MAX_M = 16         # GSR_HARMONIC_MAX_M
LEAVES = ("xyz", "t", "scaling", "scaling_t", "rotation", "rotation_r", "opacity")
_COLS = {"xyz": 3, "t": 1, "scaling": 3, "scaling_t": 1, "rotation": 4, "rotation_r": 4, "opacity": 1}


_vp, _dbl = ctypes.c_void_p, ctypes.c_double
_lib, _run = _binding.declare("gsr_slice4d.h", {
    "gsr_slice4d_forward": (ctypes.c_int, [ctypes.c_int] + [_vp] * 7 + [_dbl] * 3 + [_vp] * 5),
    "gsr_slice4d_backward": (ctypes.c_int, [ctypes.c_int] + [_vp] * 7 + [_dbl] * 3 + [_vp] * 12),
    "gsr_harmonic_features": (ctypes.c_int, [ctypes.c_int] * 3 + [_vp, _vp, _dbl, _dbl, _vp, _vp]),
    "gsr_harmonic_features_backward": (ctypes.c_int, [ctypes.c_int] * 3 + [_vp, _vp, _dbl, _dbl, _vp, _vp, _vp, _vp]),
})
_ptr, _number = _binding.ptr, _binding.check_number
_check_device = functools.partial(_binding.check_device, "4D slice kernels")


def _features_shape(n, t, P):
    if t.dim() != 4 or t.shape[0] != P or P < 1 or t.shape[3] != 3 or not 1 <= t.shape[1] <= MAX_N + 1 or not 1 <= t.shape[2] <= MAX_M:
        raise RuntimeError(f"features_t must be (P, N + 1, M, 3) with P >= 1, 0 <= N <= {MAX_N} and 1 <= M <= {MAX_M}; got {tuple(t.shape)}")


def _check(**named):
    """Every refusal of the tensors a call names (the seven leaves by their names; features_t (P, N+1, M, 3)) but the device's, before
    the kernel library is touched.  -> P"""
    return _binding.check_rows(list(named.items()), _COLS, _features_shape)


def _check_scalars(time, scaling_modifier, cutoff):
    time, m, c = _number("time", time), _number("scaling_modifier", scaling_modifier), _number("cutoff", cutoff)
    if not math.isfinite(time):
        raise ValueError(f"time must be finite; got {time}")
    if not (math.isfinite(m) and m > 0.0):
        raise ValueError(f"scaling_modifier must be finite and positive; got {m}")
    if not 0.0 <= c < 1.0:
        raise ValueError(f"cutoff must lie in [0, 1); got {c}")
    return time, m, c


class _SliceAt(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, t, scaling, scaling_t, rotation, rotation_r, opacity, time, modifier, cutoff, velocity):
        leaves = (xyz, t, scaling, scaling_t, rotation, rotation_r, opacity)
        dev = xyz.device
        P = int(xyz.shape[0])
        with torch.cuda.device(dev):
            c = [x.detach().contiguous() for x in leaves]
            means, cov, opac = torch.empty_like(c[0]), torch.empty((P, 6), dtype=torch.float32, device=dev), torch.empty_like(c[6])
            vel = torch.empty_like(c[0]) if velocity else None
            _run("gsr_slice4d_forward", P, *(x.data_ptr() for x in c), time, modifier, cutoff, means.data_ptr(), cov.data_ptr(), opac.data_ptr(),
                 _ptr(vel), torch.cuda.current_stream(dev).cuda_stream)
        ctx.save_for_backward(*leaves)        # the backward recomputes the rest
        ctx.scalars = (time, modifier, cutoff)
        ctx.set_materialize_grads(False)      # an absent upstream gradient stays absent: NULL for the kernel
        return (means, cov, opac, vel) if velocity else (means, cov, opac)

    @staticmethod
    def backward(ctx, g_means, g_cov, g_opac, g_vel=None):
        leaves = ctx.saved_tensors
        need = ctx.needs_input_grad[:7]
        none = (None,) * 11
        if all(g is None for g in (g_means, g_cov, g_opac, g_vel)) or not any(need):
            return none
        dev = leaves[0].device
        P = int(leaves[0].shape[0])
        with torch.cuda.device(dev):
            c = [x.detach().contiguous() for x in leaves]
            gin = [None if g is None else g.to(torch.float32).contiguous() for g in (g_means, g_cov, g_opac, g_vel)]
            out = [torch.empty_like(x) if n else None for x, n in zip(c, need)]
            _run("gsr_slice4d_backward", P, *(x.data_ptr() for x in c), *ctx.scalars, *(_ptr(g) for g in gin), *(_ptr(o) for o in out),
                 torch.cuda.current_stream(dev).cuda_stream)
        return (*out, None, None, None, None)


def slice_at(xyz, t, scaling, scaling_t, rotation, rotation_r, opacity, time, scaling_modifier=1.0, cutoff=0.05, velocity=False):
    """The 4D Gaussians conditioned on t = time -> (means3D (P,3), cov3D (P,6), opacities (P,1)[, velocity (P,3)]), differentiable
    w.r.t. all seven leaves: xyz (P,3), t (P,1), scaling (P,3) and scaling_t (P,1) (log), rotation (P,4) = raw l and rotation_r (P,4) =
    raw r (both (w,x,y,z)), opacity (P,1) (logit); float32 on the device, any strides.  `time` is a Python float and gets no gradient.

    A 4-vector (x, y, z, t) is the quaternion t + x i + y j + z k; with l^ = l / |l|, r^ = r / |r| the rotation is R v = l^ v conj(r^),
    in the (x, y, z, t) ordering R = L(l^) M(r^) with the two matrices of include/gsr_slice4d.h.  Every rotation of SO(4) is reached,
    and rotation_r = rotation is the static case blockdiag(R3(rotation), 1).  A checkpoint trained with another parametrisation of the
    two quaternions (another component order, or the other isoclinic pairing) must be converted by the caller; nothing is guessed here.

        s_k = scaling_modifier exp(log-scale_k), Sigma = R diag(s^2) R^T, velocity = Sigma[:3,3] / Sigma_tt, D = time - t
        means3D   = xyz + velocity D
        cov3D     = Sigma[:3,:3] - Sigma[:3,3] Sigma[3,:3] / Sigma_tt as (xx, xy, xz, yy, yz, zz): the rasterizer's cov3D_precomp
        opacities = sigmoid(opacity) exp(-D^2 / (2 Sigma_tt)) where the temporal marginal exceeds `cutoff` (0.05: the paper's rule),
                    elsewhere exactly 0: the row is masked, and every one of its seven leaf gradients is exactly 0

    Evaluated in double from the float32 leaves and rounded once: the covariance is a difference of terms up to 10^4 times its size,
    which the stock float32 sequence loses.  One launch forward, one backward; the backward recomputes the forward's values."""
    named = dict(xyz=xyz, t=t, scaling=scaling, scaling_t=scaling_t, rotation=rotation, rotation_r=rotation_r, opacity=opacity)
    _check(**named)
    time, m, c = _check_scalars(time, scaling_modifier, cutoff)
    if not isinstance(velocity, bool):
        raise TypeError(f"velocity must be True or False, got {velocity!r}")
    _check_device(*named.values())
    return _SliceAt.apply(xyz, t, scaling, scaling_t, rotation, rotation_r, opacity, time, m, c, velocity)


def _check_period(period):
    period = _number("period", period)
    if not (math.isfinite(period) and period > 0.0):
        raise ValueError(f"period must be finite and positive; got {period}")
    return period


class _Harmonic(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features_t, t, time, period):
        dev = features_t.device
        P, N, M = int(features_t.shape[0]), int(features_t.shape[1]) - 1, int(features_t.shape[2])
        with torch.cuda.device(dev):
            f, tt = features_t.detach().contiguous(), t.detach().contiguous()
            shs = torch.empty((P, M, 3), dtype=torch.float32, device=dev)
            _run("gsr_harmonic_features", P, N, M, f.data_ptr(), tt.data_ptr(), time, period, shs.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        ctx.save_for_backward(features_t, t)
        ctx.scalars = (time, period)
        ctx.set_materialize_grads(False)
        return shs

    @staticmethod
    def backward(ctx, g_shs):
        features_t, t = ctx.saved_tensors
        need_f, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g_shs is None or not (need_f or need_t):
            return None, None, None, None
        dev = features_t.device
        P, N, M = int(features_t.shape[0]), int(features_t.shape[1]) - 1, int(features_t.shape[2])
        with torch.cuda.device(dev):
            f, tt, g = features_t.detach().contiguous(), t.detach().contiguous(), g_shs.to(torch.float32).contiguous()
            d_f = torch.empty_like(f) if need_f else None
            d_t = torch.empty_like(tt) if need_t else None
            _run("gsr_harmonic_features_backward", P, N, M, f.data_ptr(), tt.data_ptr(), *ctx.scalars, g.data_ptr(), _ptr(d_f), _ptr(d_t),
                 torch.cuda.current_stream(dev).cuda_stream)
        return d_f, d_t, None, None


def harmonic_features(features_t, t, time, period):
    """SH coefficients modulated by a Fourier series in time - t -> shs (P, M, 3), differentiable w.r.t. features_t and t.
    features_t (P, N + 1, M, 3) holds N <= 3 temporal harmonics of M <= 16 SH coefficients; t (P, 1); float32 on the device, any strides;
    `time` and `period` are Python floats.  shs[i] = sum_n c_n(i) features_t[i, n] with c_n = fp32(cos(2 pi n (time - t_i) / period)),
    argument and cosine in double, the sum one float32 fma chain in ascending n started at features_t[i, 0]; N = 0 returns harmonic 0
    bit for bit.  dL/dt_i is accumulated in double in a fixed order by one owner per Gaussian: no atomics."""
    _check(t=t, features_t=features_t)
    time = _number("time", time)
    if not math.isfinite(time):
        raise ValueError(f"time must be finite; got {time}")
    period = _check_period(period)
    _check_device(features_t, t)
    return _Harmonic.apply(features_t, t, time, period)


def visible_at(opacities):
    """The mask 4DGS culls by: opacities > 0 (P,) bool of slice_at()'s opacities (P,1) -- False exactly where the temporal marginal is at
    or below the cutoff (a sigmoid that underflows to 0 in float32 counts as invisible too)."""
    if not torch.is_tensor(opacities) or opacities.dim() != 2 or opacities.shape[1] != 1:
        raise RuntimeError("opacities must be the (P, 1) tensor of slice_at()")
    return opacities.detach()[:, 0] > 0
