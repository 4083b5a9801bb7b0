"""GPU: the hash-grid encoding (include/gsr_hashgrid.h, csrc/hashgrid.hip, fused_hashgrid) against the references of
tests/torch_hashgrid.py, whose fixtures tests/test_hashgrid_cpu.py validates.  Raw calls write into buffers with canary elements
behind and between the rows of every output.

Integer fixtures are exact (array_equal): they pin the cells, the dense index and the hash, the corner order and the alias at the top
cell.  General fixtures: every decided element of y equals the float32 chain emulation bit for bit; EVERY element of dtable equals the
int64 emulation bit for bit; dx lies within 2^-24 |ref| + 2^-40 sum |terms| of the float64 rule on the rows that are not fragile.  Each
bar is printed as achieved / bound before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
import torch_hashgrid as th

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CANARY = 12345.0
_cache = {}


class Guarded:
    """A (rows, cols) float32 view with row stride cols + pad inside a buffer filled with canaries, and 64 of them behind it"""

    def __init__(self, rows, cols, pad=0, data=None):
        self.stride = cols + pad
        self.buf = torch.full((rows * self.stride + 64,), CANARY, dtype=torch.float32, device=DEV)
        self.view = self.buf[:rows * self.stride].view(rows, self.stride)[:, :cols]
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data, np.float32)))

    def ptr(self):
        return self.buf.data_ptr()

    def numpy(self):
        """The view's values, after checking that nothing outside it was written"""
        rest = self.buf.clone()
        rest[:self.view.shape[0] * self.stride].view(self.view.shape[0], self.stride)[:, :self.view.shape[1]] = CANARY
        assert bool((rest == CANARY).all()), "a canary was overwritten"
        return self.view.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def raw(case, *, N=None, pad=0, want=("dx", "dtable"), scratch="full", dy=None, x=None, backward=True):
    """The two entry points on a fixture -> dict(y, dx, dtable) of numpy arrays; what is not wanted is None (and was left untouched).
    scratch: "full", "min" or a number of bytes"""
    import fused_hashgrid as fh
    cfg = case["cfg"]
    D, L, F, T, base, pls = cfg
    x = case["x"] if x is None else x
    dy = case["dy"] if dy is None else dy
    N = x.shape[0] if N is None else N
    x, dy = x[:N], dy[:N]
    total = th.layout(cfg)["total"]
    d = fh.HashGridDesc(N=N, D=D, L=L, F=F, base_resolution=base, per_level_scale=pls, log2_hashmap_size=T)
    gx, gdy = Guarded(N, D, pad, x), Guarded(N, L * F, pad, dy)
    gy, gdx, gdt = Guarded(N, L * F, pad), Guarded(N, D, pad), Guarded(total, F)
    d.x_stride, d.dx_stride, d.y_stride, d.dy_stride = gx.stride, gdx.stride, gy.stride, gdy.stride
    table = torch.from_numpy(case["table"]).to(DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    fh._run("gsr_hashgrid_forward", ctypes.byref(d), gx.ptr(), table.data_ptr(), gy.ptr(), stream)
    out = dict(y=gy.numpy(), dx=None, dtable=None)
    if backward:
        lo, full = ctypes.c_size_t(), ctypes.c_size_t()
        fh._run("gsr_hashgrid_scratch_bytes", ctypes.byref(d), ctypes.byref(lo), ctypes.byref(full))
        nbytes = full.value if scratch == "full" else lo.value if scratch == "min" else int(scratch)
        sbuf = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device=DEV)   # contents irrelevant; 256 guard bytes behind
        fh._run("gsr_hashgrid_backward", ctypes.byref(d), gx.ptr(), table.data_ptr(), gdy.ptr(), gdx.ptr() if "dx" in want else None,
                gdt.ptr() if "dtable" in want else None, sbuf.data_ptr(), nbytes, stream)
        torch.cuda.synchronize()
        assert bool((sbuf[nbytes:] == 0x5A).all()), "the scratch was overrun"
        dxv, dtv = gdx.numpy(), gdt.numpy()
        out["dx"] = dxv if "dx" in want else None
        out["dtable"] = dtv if "dtable" in want else None
        if "dx" not in want:
            assert (dxv == CANARY).all()
        if "dtable" not in want:
            assert (dtv == CANARY).all()
    return out


def fixture(name, kind):
    key = (name, kind)
    if key not in _cache:
        _cache[key] = th.integer_fixture(name) if kind == "integer" else th.general_fixture(name)
    return _cache[key]


def refs(case, N=None, dy=None):
    """emulate_y, emulate_dtable and ref64 of a fixture (its first N rows, another dy), computed once"""
    key = ("refs", id(case), N, None if dy is None else id(dy))
    if key not in _cache:
        x, g = case["x"][:N], (case["dy"] if dy is None else dy)[:N]
        y, und = th.emulate_y(x, case["table"], case["cfg"])
        dt, q, n_e = th.emulate_dtable(x, g, case["cfg"], info=True)
        _cache[key] = (case, dy, dict(y=y, und=und, dtable=dt, q=q, n_e=n_e, r64=th.ref64(x, case["table"], g, case["cfg"]),
                                      fragile=th.fragile_rows(x, case["cfg"])))
    return _cache[key][2]


def check_general(got, ref, what):
    dec = ~ref["und"]
    assert np.array_equal(bits(got["y"])[dec], bits(ref["y"])[dec]), (what, "y")
    if got["dtable"] is not None:
        bad = np.argwhere(bits(got["dtable"]) != bits(ref["dtable"]))
        assert len(bad) == 0, (what, "dtable", bad[:4])
    if got["dx"] is not None:
        ok = ~ref["fragile"]
        r = ref["r64"]
        bound = 2.0 ** -24 * np.abs(r["dx"]) + 2.0 ** -40 * r["dx_abs"]
        err = np.abs(got["dx"].astype(np.float64) - r["dx"])
        worst = float((err[ok] / np.maximum(bound[ok], 1e-300)).max()) if ok.any() and err[ok].max() > 0 else 0.0
        print(f"{what}: dx achieved / bound = {worst:.3f} (max err {err[ok].max() if ok.any() else 0:.3e}; {int((~ok).sum())} fragile rows left out)")
        assert (err[ok] <= bound[ok]).all(), (what, "dx", worst)


def check_table_bound(got, ref, what):
    """|dtable - float64 sum| <= n_e 2^-(q+1) + one float32 rounding (the header's bound), plus the float64 reference's own error"""
    r = ref["r64"]
    bound = ref["n_e"][:, None] * 2.0 ** -(ref["q"] + 1) + 2.0 ** -24 * np.abs(r["dtable"]) + 2.0 ** -50 * r["dtable_abs"] + 2.0 ** -149
    err = np.abs(got["dtable"].astype(np.float64) - r["dtable"])
    worst = float((err / bound).max())
    print(f"{what}: dtable against the float64 sum, achieved / bound = {worst:.3f} (max err {err.max():.3e}, q = {ref['q']})")
    assert (err <= bound).all(), (what, worst)


# ---- the fixtures reach every path ---------------------------------------------------------------------------------------------------
def test_fixtures_reach_both_paths_and_the_seams():
    import fused_hashgrid as fh
    D, L, F, T, base, pls = th.CONFIGS["all3"]
    off, res, hashed, total = fh.level_layout(D, L, F, T, base, pls)
    paths = fh.level_paths(D, L, F, T, base, pls)
    assert res == [2, 4, 8, 16, 32] and hashed == [False, False, False, False, True]
    assert res[3] ** 3 == off[4] - off[3] == 1 << T                                    # dense with res^D == size exactly, the next one hashed
    assert paths == [fh.PATH_LDS] * 3 + [fh.PATH_DIRECT] * 2                           # a dense level on each side of the LDS budget
    assert off[1] - off[0] == 8                                                        # 1000 x 8 terms into 8 entries
    D, L, F, T, base, pls = th.CONFIGS["tiny2"]
    off, res, hashed, total = fh.level_layout(D, L, F, T, base, pls)
    assert [b - a for a, b in zip(off, off[1:])] == [8, 16, 16] and hashed == [False, False, True]   # 16-entry levels, dense and hashed
    D, L, F, T, base, pls = th.CONFIGS["budget2"]
    assert fh.level_paths(D, L, F, T, base, pls) == [fh.PATH_LDS, fh.PATH_DIRECT, fh.PATH_DIRECT]
    assert fh.level_layout(D, L, F, T, base, pls)[2] == [False, False, True]
    seen = set()
    for cfg in th.CONFIGS.values():
        seen |= set(fh.level_paths(*cfg))
    assert seen == {fh.PATH_LDS, fh.PATH_DIRECT}


# ---- integer fixtures: exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", th.INTEGER_CONFIGS)
def test_integer_fixtures_are_exact(name):
    c = fixture(name, "integer")
    r = th.ref64(c["x"], c["table"], c["dy"], c["cfg"])
    got = raw(c, pad=th.INTEGER_CONFIGS.index(name) % 4)
    for k in ("y", "dtable", "dx"):
        assert np.array_equal(got[k], r[k].astype(np.float32)), (name, k, np.argwhere(got[k] != r[k].astype(np.float32))[:4])


# ---- general fixtures --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(th.CONFIGS))
def test_general_fixtures(name):
    c = fixture(name, "general")
    ref = refs(c)
    got = raw(c, pad=sorted(th.CONFIGS).index(name) % 3)
    check_general(got, ref, name)
    check_table_bound(got, ref, name)


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 257, 1000])
def test_row_counts(N):
    c = fixture("all3", "general")
    got = raw(c, N=N, pad=1)
    if N == 0:
        assert got["y"].shape == (0, 40) and got["dx"].shape == (0, 3)
        assert not bits(got["dtable"]).any()   # a backward with N == 0 writes +0
        return
    check_general(got, refs(c, N), f"all3 N={N}")


@pytest.mark.parametrize("name", ["seam3", "hashed4", "dense2"])
def test_row_counts_across_dimensions(name):
    c = fixture(name, "general")
    for N in (1, 65):
        check_general(raw(c, N=N), refs(c, N), f"{name} N={N}")


# ---- reproducibility and invariance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all3", "budget2", "hashed4"])
def test_row_permutation_scratch_size_and_repeats_change_no_bit(name):
    c = fixture(name, "general")
    a = raw(c)
    perm = np.random.default_rng(11).permutation(len(c["x"]))
    b = raw(c, x=c["x"][perm], dy=c["dy"][perm])
    assert np.array_equal(bits(a["dtable"]), bits(b["dtable"]))
    assert np.array_equal(bits(a["y"])[perm], bits(b["y"])) and np.array_equal(bits(a["dx"])[perm], bits(b["dx"]))
    again = raw(c)
    small = raw(c, scratch="min")
    import fused_hashgrid as fh
    lay = th.layout(c["cfg"])
    two = 256 + (lay["sizes"][-1] + lay["sizes"][-2]) * c["cfg"][2] * 8   # room for two of the last levels, not for everything
    middle = raw(c, scratch=two)
    for other in (again, small, middle):
        for k in ("y", "dx", "dtable"):
            assert np.array_equal(bits(a[k]), bits(other[k])), k
    only_dx, only_dt = raw(c, want=("dx",)), raw(c, want=("dtable",), scratch="min")
    assert only_dx["dtable"] is None and np.array_equal(bits(only_dx["dx"]), bits(a["dx"]))
    assert only_dt["dx"] is None and np.array_equal(bits(only_dt["dtable"]), bits(a["dtable"]))
    assert fh.level_paths(*c["cfg"])   # (the layout call itself: host only)


# ---- edge cases ------------------------------------------------------------------------------------------------------------------------
def test_void_rows_and_coordinates_outside_the_unit_cube():
    c = fixture("all3", "general")
    x = c["x"]
    void = ~np.isfinite(x).all(1)
    outside = (x < 0) | (x > 1)
    assert void.sum() == 3 and (outside & ~void[:, None]).sum() >= 3
    got = raw(c)
    assert not bits(got["y"])[void].any() and not bits(got["dx"])[void].any()          # +0, bit for bit
    assert not bits(got["dx"])[outside & ~void[:, None]].any()                         # a clamped axis has exactly +0
    # the same rows replaced by ordinary ones: every other row keeps its bits
    x2 = x.copy()
    special = void | outside.any(1)
    x2[special] = 0.5
    other = raw(c, x=x2)
    assert np.array_equal(bits(got["y"])[~special], bits(other["y"])[~special])
    assert np.array_equal(bits(got["dx"])[~special], bits(other["dx"])[~special])
    # clamping: x = -3 reads as 0 and x = 1.5 as 1
    x3 = np.clip(np.where(void[:, None], 0.5, x), 0, 1).astype(np.float32)
    clamped = raw(c, x=x3, want=())
    rows_out = outside.any(1) & ~void
    assert np.array_equal(bits(got["y"])[rows_out], bits(clamped["y"])[rows_out])


def test_an_infinite_gradient_makes_the_table_gradient_nan_and_a_zero_one_zero():
    c = fixture("seam3", "general")
    for bad in (np.inf, np.nan):
        dy = c["dy"].copy()
        dy[700, 3] = bad
        got = raw(c, dy=dy, want=("dtable",))
        assert np.isnan(got["dtable"]).all()
    dy = c["dy"].copy()
    dy[9] = np.inf                                       # a void row's dy counts in the maximum all the same (the header's m)
    assert np.isnan(raw(c, dy=dy, want=("dtable",), scratch="min")["dtable"]).all()
    zero = raw(c, dy=np.zeros_like(c["dy"]))
    assert not bits(zero["dtable"]).any() and not bits(zero["dx"]).any()


@pytest.mark.parametrize("name", ["all3", "tiny2"])
def test_dy_over_sixty_binades(name):
    c = fixture(name, "general")
    key = ("spread", name)
    if key not in _cache:
        k = np.random.default_rng(21).integers(-30, 31, c["dy"].shape)
        _cache[key] = (c["dy"] * np.exp2(k)).astype(np.float32)
    dy = _cache[key]
    mag = np.abs(dy[dy != 0])
    assert mag.max() / mag.min() > 2.0 ** 60
    ref = refs(c, None, dy)
    got = raw(c, dy=dy)
    check_general(got, ref, f"{name} spread")
    check_table_bound(got, ref, f"{name} spread")
    assert np.array_equal(bits(raw(c, dy=dy, scratch="min", want=("dtable",))["dtable"]), bits(ref["dtable"]))


# ---- autograd ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all3", "budget2", "seam4"])
def test_autograd_equals_the_torch_version_in_float64(name):
    import fused_hashgrid as fh
    c = fixture(name, "general")
    D, L, F, T, base, pls = c["cfg"]
    ref = refs(c)
    x = torch.from_numpy(c["x"]).to(DEV).requires_grad_(True)
    table = torch.from_numpy(c["table"]).to(DEV).requires_grad_(True)
    g = torch.from_numpy(c["dy"]).to(DEV)
    wide = torch.cat([torch.zeros((len(c["x"]), 3), device=DEV), g, torch.zeros((len(c["x"]), 2), device=DEV)], 1)
    y = fh.hash_grid(x, table, L, F, T, base, pls)
    y.backward(wide[:, 3:3 + L * F])                     # a column slice of a wider matrix: read in place
    # the torch version in float64 on the CPU
    x64 = torch.from_numpy(c["x"]).double().requires_grad_(True)
    t64 = torch.from_numpy(c["table"]).double().requires_grad_(True)
    (th.hash_grid_torch(x64, t64, c["cfg"]) * torch.from_numpy(c["dy"]).double()).sum().backward()
    got = dict(y=y.detach().cpu().numpy(), dx=x.grad.cpu().numpy(), dtable=table.grad.cpu().numpy())
    check_general(got, ref, f"{name} autograd")
    void = ~np.isfinite(c["x"]).all(1)
    ok = ~ref["fragile"] & ~void
    dx64 = x64.grad.numpy()
    bound = 2.0 ** -24 * np.abs(dx64) + 2.0 ** -40 * ref["r64"]["dx_abs"]
    err = np.abs(got["dx"].astype(np.float64) - dx64)
    print(f"{name} autograd: x.grad achieved / bound = {float((err[ok] / np.maximum(bound[ok], 1e-300)).max()):.3f}")
    assert (err[ok] <= bound[ok]).all()
    # table.grad: the header's bound around the float64 sum (plus that sum's own rounding)
    d64 = t64.grad.numpy()
    bound = ref["n_e"][:, None] * 2.0 ** -(ref["q"] + 1) + 2.0 ** -24 * np.abs(d64) + 2.0 ** -50 * ref["r64"]["dtable_abs"] + 2.0 ** -149
    err = np.abs(got["dtable"].astype(np.float64) - d64)
    print(f"{name} autograd: table.grad achieved / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    # only what is required is formed
    x2 = torch.from_numpy(c["x"]).to(DEV)
    t2 = torch.from_numpy(c["table"]).to(DEV).requires_grad_(True)
    fh.hash_grid(x2, t2, L, F, T, base, pls).backward(g)
    assert torch.equal(t2.grad, table.grad)
    y0, dx0, dt0 = fh.hash_grid_and_grads(x2, t2, g, levels=L, features=F, log2_hashmap_size=T, base_resolution=base, per_level_scale=pls)
    assert torch.equal(y0, y.detach()) and torch.equal(dx0, x.grad) and torch.equal(dt0, table.grad)


def test_hashgrid_mlp_and_an_adam_step_repeat_bit_for_bit():
    import fused_hashgrid as fh
    import fused_mlp as fm
    from fused_params import FusedAdam
    N = 1000
    gen = torch.Generator().manual_seed(5)
    x01, dirs = torch.rand((N, 3), generator=gen).to(DEV), torch.nn.functional.normalize(torch.randn((N, 3), generator=gen), dim=1).to(DEV)
    target = torch.rand((N, 3), generator=gen).to(DEV)
    torch.manual_seed(3)
    grid = fh.HashGrid(3, levels=8, features=2, log2_hashmap_size=12, base_resolution=4, finest_resolution=128).to(DEV)
    mlp = fm.TinyMLP(grid.out_dim + 3, 3, hidden=32, hidden_layers=2, output_activation="sigmoid").to(DEV)
    with torch.no_grad():
        grid.table.mul_(1e3)   # U(-0.1, 0.1): the first step's gradients are then well above the table's rounding
    state = [p.detach().clone() for p in [grid.table] + list(mlp.parameters())]

    def step():
        params = [grid.table] + list(mlp.parameters())
        with torch.no_grad():
            for p, s in zip(params, state):
                p.copy_(s)
                p.grad = None
        loss = ((mlp(torch.cat([grid(x01), dirs], 1)) - target) ** 2).mean()
        loss.backward()
        grads = [p.grad.clone() for p in params]
        opt = FusedAdam([{"params": [grid.table], "lr": 1e-2}, {"params": list(mlp.parameters()), "lr": 1e-3}])
        opt.step()
        return float(loss), grads, [p.detach().clone() for p in params]

    loss1, g1, p1 = step()
    loss2, g2, p2 = step()
    assert np.isfinite(loss1) and loss1 == loss2
    assert float(g1[0].abs().max()) > 0
    for a, b in zip(g1 + p1, g2 + p2):
        assert torch.equal(a, b)
    for s, p in zip(state, p1):
        assert float((s - p).abs().max()) > 0   # every parameter moved
