"""Reference of the one-launch Adam (include/gsr.h gsr_adam_step, fused_params.FusedAdam) in plain tensor arithmetic, written from
its definition and not from torch.optim:

    m'    = m + (1 - b1) (g - m)
    v'    = b2 v + (1 - b2) g^2
    denom = sqrt(v') / sqrt(1 - b2^t) + eps
    p'    = p - lr / (1 - b1^t) . m' / denom                            (t = the 1-based count of this step)

dtype=torch.float64 is the truth, the same code with dtype=torch.float32 the measure of what fp32 arithmetic costs.  The state is
carried in `dtype` over the whole sequence of steps.  With `visible` (a boolean per row of dim 0) the other rows keep p, m and v:
the visible-only variant of FusedAdam.step(visible_radii=...), visible = radii > 0.
"""
import torch


def adam_steps(param, grads, lrs, betas=(0.9, 0.999), eps=1e-15, exp_avg=None, exp_avg_sq=None, step0=0, visible=None,
               dtype=torch.float64):
    """param: the fp32 parameter; grads: one fp32 gradient per step; lrs: one learning rate per step, or one for all; exp_avg,
    exp_avg_sq: the fp32 moments of a state that has lived `step0` steps (zeros without); visible: None, one boolean (rows,)
    tensor for all steps or one per step.  -> (param, exp_avg, exp_avg_sq) after the steps, in `dtype`."""
    b1, b2 = float(betas[0]), float(betas[1])
    conv = lambda t: t.detach().cpu().to(dtype).clone()
    p = conv(param)
    m = torch.zeros_like(p) if exp_avg is None else conv(exp_avg)
    v = torch.zeros_like(p) if exp_avg_sq is None else conv(exp_avg_sq)
    if not isinstance(lrs, (list, tuple)):
        lrs = [lrs] * len(grads)
    if visible is None or torch.is_tensor(visible):
        visible = [visible] * len(grads)
    assert len(lrs) == len(grads) == len(visible)
    for i, (g, lr, vis) in enumerate(zip(grads, lrs, visible)):
        t = int(step0) + i + 1
        g = conv(g)
        m1 = m + (1.0 - b1) * (g - m)
        v1 = b2 * v + (1.0 - b2) * (g * g)
        denom = v1.sqrt() / (1.0 - b2 ** t) ** 0.5 + eps
        p1 = p - (float(lr) / (1.0 - b1 ** t)) * (m1 / denom)
        if vis is not None:
            keep = ~vis.cpu().bool().reshape((-1,) + (1,) * (p.dim() - 1))
            p1, m1, v1 = torch.where(keep, p, p1), torch.where(keep, m, m1), torch.where(keep, v, v1)
        p, m, v = p1, m1, v1
    return p, m, v
