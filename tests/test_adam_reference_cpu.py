"""CPU: tests/torch_adam.py, the float64 restatement of Adam that tests/test_adam_gpu.py measures the HIP kernel against, pinned to
torch.optim.Adam on float64 CPU parameters (the two share no code: the reference is plain tensor arithmetic)."""
import pytest
import torch

import torch_adam

LRS = (1.6e-4, 1.6e-4, 1.6e-4, 0.9e-4, 0.9e-4, 0.9e-4)   # an lr change between steps


def _problem(seed, shape=(37, 15, 3)):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(shape, generator=g)
    grads = [torch.randn(shape, generator=g) * 10 ** float(torch.randint(-6, 1, (1,), generator=g)) for _ in LRS]
    grads[4] = torch.zeros(shape)    # a zero-gradient step: the momentum still moves the parameter
    m = 1e-3 * torch.randn(shape, generator=g)
    v = 1e-5 * torch.rand(shape, generator=g)
    return p, grads, m, v


@pytest.mark.parametrize("step0", (0, 999, 29999))
def test_float64_reference_equals_torch_optim_adam_in_float64(step0):
    p, grads, m, v = _problem(5 + step0)
    if step0 == 0:
        m, v = torch.zeros_like(m), torch.zeros_like(v)
    q = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.Adam([q], lr=LRS[0], eps=1e-15)
    opt.state[q] = {"step": torch.tensor(float(step0)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
    for lr, g in zip(LRS, grads):
        opt.param_groups[0]["lr"] = lr
        q.grad = g.double().clone()
        opt.step()
    assert int(opt.state[q]["step"]) == step0 + len(LRS)
    rp, rm, rv = torch_adam.adam_steps(p, grads, list(LRS), exp_avg=m, exp_avg_sq=v, step0=step0, dtype=torch.float64)
    assert rp.dtype == torch.float64 and float((rp - p.double()).abs().max()) > 1e-5    # it moved
    for name, a, b in (("param", rp, q.data), ("exp_avg", rm, opt.state[q]["exp_avg"]), ("exp_avg_sq", rv, opt.state[q]["exp_avg_sq"])):
        err = float((a - b).abs().max())
        print(f"step0 {step0} {name}: max|reference - torch.optim.Adam| = {err:.2e}")
        assert err <= 1e-12, (name, err)


def test_other_betas_and_eps_and_the_float32_run():
    p, grads, m, v = _problem(77, (50, 4))
    q = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.Adam([q], lr=1e-3, betas=(0.8, 0.99), eps=1e-8)
    for g in grads:
        q.grad = g.double().clone()
        opt.step()
    rp, rm, rv = torch_adam.adam_steps(p, grads, 1e-3, betas=(0.8, 0.99), eps=1e-8)
    assert float((rp - q.data).abs().max()) <= 1e-12
    assert float((rm - opt.state[q]["exp_avg"]).abs().max()) <= 1e-12 and float((rv - opt.state[q]["exp_avg_sq"]).abs().max()) <= 1e-12
    fp, fm, fv = torch_adam.adam_steps(p, grads, 1e-3, betas=(0.8, 0.99), eps=1e-8, dtype=torch.float32)
    assert fp.dtype == fm.dtype == fv.dtype == torch.float32
    n32 = float((fp.double() - rp).abs().max() / rp.abs().max())
    assert 0.0 < n32 < 1e-6, n32       # fp32 state: a few ulps of the largest element, and not the float64 run again


def test_invisible_rows_keep_parameter_and_moments():
    p, grads, m, v = _problem(9, (37, 3))
    vis = torch.zeros(37, dtype=torch.bool)
    vis[::2] = True
    dp, dm, dv = torch_adam.adam_steps(p, grads, 1e-3, exp_avg=m, exp_avg_sq=v, step0=999)
    rp, rm, rv = torch_adam.adam_steps(p, grads, 1e-3, exp_avg=m, exp_avg_sq=v, step0=999, visible=vis)
    for got, dense, before in ((rp, dp, p), (rm, dm, m), (rv, dv, v)):
        assert torch.equal(got[~vis], before.double()[~vis]) and torch.equal(got[vis], dense[vis])
    # one mask per step: a row seen in the last step alone has taken that step alone, from the state it had
    masks = [torch.zeros(37, dtype=torch.bool) for _ in grads]
    masks[-1][3] = True
    sp, sm, sv = torch_adam.adam_steps(p, grads, 1e-3, exp_avg=m, exp_avg_sq=v, step0=999, visible=masks)
    op, om, ov = torch_adam.adam_steps(p[3:4], [grads[-1][3:4]], 1e-3, exp_avg=m[3:4], exp_avg_sq=v[3:4], step0=999 + len(grads) - 1)
    assert torch.equal(sp[3:4], op) and torch.equal(sm[3:4], om) and torch.equal(sv[3:4], ov)
    assert torch.equal(sp[4:], p.double()[4:])
