"""GPU: the plane-grid encoding (include/gsr_hexplane.h, csrc/hexplane.hip, fused_hexplane) against the references of
tests/torch_hexplane.py, whose fixtures tests/test_hexplane_cpu.py validates.  Raw calls write into buffers with canary elements
behind and between the rows of every output.

Integer fixtures are exact (array_equal): they pin the planes' order and axes, the corner order and the top node.  General fixtures:
every decided element of y equals the float32 emulation bit for bit; EVERY element of dtable equals the int64 emulation bit for bit;
dx lies within 2^-24 |ref| + 2^-40 sum |terms| of the float64 rule.  Each bar is printed as achieved / bound before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
import torch_hexplane as th

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
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data, np.float32).reshape(rows, cols)))

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


def config(c):
    import fused_hexplane as fh
    return fh.HexPlaneConfig(c.D, c.C, c.res, c.concat)


def raw(case, *, N=None, pad=0, want=("dx", "dtable"), scratch="full", dy=None, x=None, table=None, backward=True):
    """The two entry points on a fixture -> dict(y, dx, dtable) of numpy arrays; what is not wanted is None (and was left untouched).
    scratch: "full", "min" or a number of bytes"""
    import fused_hexplane as fh
    c = case["cfg"]
    x = case["x"] if x is None else x
    dy = case["dy"] if dy is None else dy
    table = case["table"] if table is None else table
    N = x.shape[0] if N is None else N
    x, dy = x[:N], dy[:N]
    cols, total = th.out_dim(c), th.total(c)
    d = config(c).desc(N)
    gx, gdy = Guarded(N, c.D, pad, x), Guarded(N, cols, pad, dy)
    gy, gdx, gdt = Guarded(N, cols, pad), Guarded(N, c.D, pad), Guarded(1, total)
    d.x_stride, d.dx_stride, d.y_stride, d.dy_stride = gx.stride, gdx.stride, gy.stride, gdy.stride
    tab = torch.from_numpy(table).to(DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    fh._run("gsr_hexplane_forward", ctypes.byref(d), gx.ptr(), tab.data_ptr(), gy.ptr(), stream)
    out = dict(y=gy.numpy(), dx=None, dtable=None)
    if backward:
        lo, full = ctypes.c_size_t(), ctypes.c_size_t()
        fh._run("gsr_hexplane_scratch_bytes", ctypes.byref(d), ctypes.byref(lo), ctypes.byref(full))
        nbytes = full.value if scratch == "full" else lo.value if scratch == "min" else int(scratch)
        sbuf = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device=DEV)   # contents irrelevant; 256 guard bytes behind
        fh._run("gsr_hexplane_backward", ctypes.byref(d), gx.ptr(), tab.data_ptr(), gdy.ptr(), gdx.ptr() if "dx" in want else None,
                gdt.ptr() if "dtable" in want else None, sbuf.data_ptr(), nbytes, stream)
        torch.cuda.synchronize()
        assert bool((sbuf[nbytes:] == 0x5A).all()), "the scratch was overrun"
        dxv, dtv = gdx.numpy(), gdt.numpy()[0]
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
        _cache[key] = {"integer": th.integer_fixture, "general": th.general_fixture, "one_cell": th.one_cell_fixture}[kind](name)
    return _cache[key]


def refs(case, N=None, dy=None, table=None):
    """emulate_y, emulate_dtable and ref64 of a fixture (its first N rows, another dy or table), computed once"""
    key = ("refs", id(case), N, None if dy is None else id(dy), None if table is None else id(table))
    if key not in _cache:
        x, g, t = case["x"][:N], (case["dy"] if dy is None else dy)[:N], case["table"] if table is None else table
        y, und, _ = th.emulate_y(x, t, case["cfg"])
        dt, q, n_e, worst = th.emulate_dtable(x, t, g, case["cfg"], info=True)
        _cache[key] = (case, dy, table, dict(y=y, und=und, dtable=dt, q=q, n_e=n_e, r64=th.ref64(x, t, g, case["cfg"])))
    return _cache[key][3]


def check_general(got, ref, what):
    dec = ~ref["und"]
    assert np.array_equal(bits(got["y"])[dec], bits(ref["y"])[dec]), (what, "y", np.argwhere(bits(got["y"]) != bits(ref["y"]))[:4])
    if got["dtable"] is not None:
        bad = np.argwhere(bits(got["dtable"]) != bits(ref["dtable"]))
        assert len(bad) == 0, (what, "dtable", bad[:4])
    if got["dx"] is not None:
        r = ref["r64"]
        bound = 2.0 ** -24 * np.abs(r["dx"]) + 2.0 ** -40 * r["dx_abs"]
        err = np.abs(got["dx"].astype(np.float64) - r["dx"])
        worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size and err.max() > 0 else 0.0
        print(f"{what}: dx achieved / bound = {worst:.3f} (max err {err.max() if err.size else 0:.3e})")
        assert (err <= bound).all(), (what, "dx", worst)


def check_table_bound(got, ref, cfg, what):
    """|dtable - float64 sum| <= n_e 2^-(q+1) + one float32 rounding (the header's bound), plus the float64 reference's own error"""
    r = ref["r64"]
    off, P, C = th.offsets(cfg), len(th.planes(cfg)), cfg.C
    quantum = np.zeros(off[-1])
    for j in range(len(off) - 1):
        q = ref["q"][j // P][j % P]
        quantum[off[j]:off[j + 1]] = 0.0 if q is None else 2.0 ** -(q + 1)
    bound = np.repeat(ref["n_e"], C) * quantum + 2.0 ** -24 * np.abs(r["dtable"]) + 2.0 ** -49 * r["dtable_abs"] + 2.0 ** -149
    err = np.abs(got["dtable"].astype(np.float64) - r["dtable"])
    worst = float((err / bound).max())
    print(f"{what}: dtable against the float64 sum, achieved / bound = {worst:.3f} (max err {err.max():.3e})")
    assert (err <= bound).all(), (what, worst)


# ---- the fixtures reach every path ---------------------------------------------------------------------------------------------------
def test_fixtures_reach_both_paths_and_the_seam():
    import fused_hexplane as fh
    L, Dr = fh.PATH_LDS, fh.PATH_DIRECT
    assert fh.level_paths(config(th.CONFIGS["seam_d4"])) == [[L] * 6, [Dr] + [L] * 5]      # 64 x 64 nodes: LDS; 65 x 64: direct
    assert fh.level_paths(config(th.CONFIGS["direct_d3"])) == [[Dr, L, L], [L, L, L]]
    assert fh.level_paths(config(th.CONFIGS["direct_d4"]))[0][0] == Dr and fh.level_paths(config(th.INTEGER_CONFIGS["int_seam"])) == [[Dr, L, L]]
    for name, c in th.CONFIGS.items():
        assert fh.level_paths(config(c)) == [[L if v else Dr for v in level] for level in th.lds(c)], name


# ---- integer fixtures: exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(th.INTEGER_CONFIGS))
def test_integer_fixtures_are_exact(name):
    c = fixture(name, "integer")
    r = th.ref64(c["x"], c["table"], c["dy"], c["cfg"])
    got = raw(c, pad=sorted(th.INTEGER_CONFIGS).index(name))
    for k in ("y", "dtable", "dx"):
        assert np.array_equal(got[k], r[k].astype(np.float32)), (name, k, np.argwhere(got[k] != r[k].astype(np.float32))[:4])


# ---- general fixtures --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(th.CONFIGS))
def test_general_fixtures(name):
    c = fixture(name, "general")
    ref = refs(c)
    got = raw(c, pad=sorted(th.CONFIGS).index(name) % 3)
    check_general(got, ref, name)
    check_table_bound(got, ref, c["cfg"], name)


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 257, 1000])
def test_row_counts(N):
    c = fixture("direct_d4", "general")
    got = raw(c, N=N, pad=1)
    if N == 0:
        assert got["y"].shape == (0, 64) and got["dx"].shape == (0, 4)
        assert not bits(got["dtable"]).any()   # a backward with N == 0 writes +0
        return
    check_general(got, refs(c, N), f"direct_d4 N={N}")


@pytest.mark.parametrize("name", ["multi_d3", "seam_d4", "direct_d3"])
def test_row_counts_across_shapes(name):
    c = fixture(name, "general")
    for N in (1, 65):
        check_general(raw(c, N=N), refs(c, N), f"{name} N={N}")


@pytest.mark.parametrize("name", ["seam_d4", "direct_d3"])
def test_a_thousand_rows_in_one_cell(name):
    """A hot node on both paths: a thousand terms meet in each of four nodes of every plane of level 0"""
    c = fixture(name, "one_cell")
    ref = refs(c)
    assert int(ref["n_e"].max()) == 1000
    got = raw(c)
    check_general(got, ref, f"{name} one cell")
    check_table_bound(got, ref, c["cfg"], f"{name} one cell")


# ---- reproducibility and invariance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["seam_d4", "direct_d4", "multi_d3"])
def test_row_permutation_scratch_size_and_repeats_change_no_bit(name):
    c = fixture(name, "general")
    a = raw(c)
    perm = np.random.default_rng(11).permutation(len(c["x"]))
    b = raw(c, x=c["x"][perm], dy=c["dy"][perm])
    assert np.array_equal(bits(a["dtable"]), bits(b["dtable"]))
    assert np.array_equal(bits(a["y"])[perm], bits(b["y"])) and np.array_equal(bits(a["dx"])[perm], bits(b["dx"]))
    again = raw(c)
    small = raw(c, scratch="min")
    sizes = np.diff(th.offsets(c["cfg"]))
    two = 512 + int(sizes.max() + np.sort(sizes)[-2]) * 8   # room for the two largest planes, not for everything
    assert 512 + int(sizes.max()) * 8 < two < 512 + int(sizes.sum()) * 8
    middle = raw(c, scratch=two)
    for other in (again, small, middle):
        for k in ("y", "dx", "dtable"):
            assert np.array_equal(bits(a[k]), bits(other[k])), k
    only_dx, only_dt = raw(c, want=("dx",)), raw(c, want=("dtable",), scratch="min")
    assert only_dx["dtable"] is None and np.array_equal(bits(only_dx["dx"]), bits(a["dx"]))
    assert only_dt["dx"] is None and np.array_equal(bits(only_dt["dtable"]), bits(a["dtable"]))


# ---- edge cases ------------------------------------------------------------------------------------------------------------------------
def test_void_rows_and_coordinates_on_and_beyond_the_border():
    c = fixture("odd_d4", "general")
    x = c["x"]
    void, clamped = th.rows(x)
    assert void.sum() == 3 and (clamped & ~void[:, None]).sum() >= 6
    got = raw(c)
    assert not bits(got["y"])[void].any() and not bits(got["dx"])[void].any()          # +0, bit for bit
    assert not bits(got["dx"])[clamped & ~void[:, None]].any()                         # a clamped axis has exactly +0
    # the same rows replaced by ordinary ones: every other row keeps its bits
    x2 = x.copy()
    special = void | clamped.any(1)
    x2[special] = 0.5
    other = raw(c, x=x2)
    assert np.array_equal(bits(got["y"])[~special], bits(other["y"])[~special])
    assert np.array_equal(bits(got["dx"])[~special], bits(other["dx"])[~special])
    # border padding: u = -3 reads as -1 and u = 1.5 as +1
    x3 = np.clip(np.where(void[:, None], 0.5, x), -1, 1).astype(np.float32)
    inside = raw(c, x=x3, backward=False)
    rows_out = clamped.any(1) & ~void
    assert np.array_equal(bits(got["y"])[rows_out], bits(inside["y"])[rows_out])


def test_non_finite_gradients_or_planes_make_the_table_gradient_nan_and_zeros_make_zeros():
    c = fixture("direct_d3", "general")
    for bad in (np.inf, np.nan):
        dy = c["dy"].copy()
        dy[700, 3] = bad
        assert np.isnan(raw(c, dy=dy, want=("dtable",))["dtable"]).all()
    dy = c["dy"].copy()
    dy[9] = np.inf                                       # a void row's dy counts in the maximum all the same (the header's m)
    assert np.isnan(raw(c, dy=dy, want=("dtable",), scratch="min")["dtable"]).all()
    off = th.offsets(c["cfg"])
    table = c["table"].copy()
    table[off[4] + 5] = np.nan                            # one NaN in one small plane of the last level
    assert np.isnan(raw(c, table=table, want=("dtable",))["dtable"]).all()
    zero = raw(c, dy=np.zeros_like(c["dy"]))
    assert not bits(zero["dtable"]).any() and not bits(zero["dx"]).any()
    table = c["table"].copy()
    table[off[1]:off[2]] = 0                              # an all-zero plane: +0 in the two others of its level, not in its own
    key = ("zero plane", id(c))
    if key not in _cache:
        _cache[key] = table
    table = _cache[key]
    ref = refs(c, None, None, table)
    assert ref["q"][0] == [None, ref["q"][0][1], None] and ref["q"][0][1] is not None
    got = raw(c, table=table)
    check_general(got, ref, "direct_d3 zero plane")
    assert not bits(got["dtable"])[:off[1]].any() and not bits(got["dtable"])[off[2]:off[3]].any() and got["dtable"][off[1]:off[2]].any()


@pytest.mark.parametrize("name", ["direct_d4", "odd_d4"])
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
    check_table_bound(got, ref, c["cfg"], f"{name} spread")
    assert np.array_equal(bits(raw(c, dy=dy, scratch="min", want=("dtable",))["dtable"]), bits(ref["dtable"]))


# ---- the regulariser ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [(5, 4, 3, 2), (4, 6, 2, 3), (40, 30, 5, 4)])
def test_regulariser_value_and_gradient(res):
    """res_b of the time planes 2, 3 and 4; of the space planes 2 .. 60; the last shape has planes of 1 to 19 workgroups.  The value
    and every gradient element within one float32 rounding of the float64 reference, plus that reference's own error: it and the
    kernel are two float64 evaluations, in different orders, of a sum of at most nine terms that may cancel, so an element of the
    reference is itself only good to a few 2^-53 of its largest term; 2^-50 of the largest gradient element stands for that.
    Repeats give equal bits."""
    import fused_hexplane as fh
    c = th.Cfg(4, 8, (res, tuple(2 * r if a < 3 else r for a, r in enumerate(res))), True)
    cfg = config(c)
    rng = np.random.default_rng(31)
    host = (1.0 + 0.5 * rng.standard_normal(th.total(c))).astype(np.float32)
    host[::97] = 1.0                                         # |1 - v| at its kink: the derivative is 0
    kw = dict(tv_space=0.25, tv_time=0.75, smooth_space=0.125, smooth_time=1.5, l1_time=0.5)   # float32 values: the ABI takes floats
    t64 = torch.from_numpy(host).double().requires_grad_(True)
    want = th.regularizer_torch(t64, c, **kw)
    want.backward()
    want, gwant = float(want.detach()), t64.grad.numpy()
    outs = []
    for _ in range(2):
        table = torch.from_numpy(host).to(DEV).requires_grad_(True)
        value = fh.plane_regularizer(table, cfg, **kw)
        value.backward()
        outs.append((value.detach().cpu().numpy(), table.grad.cpu().numpy()))
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])) and np.array_equal(bits(outs[0][1]), bits(outs[1][1]))
    value, grad = float(outs[0][0]), outs[0][1].astype(np.float64)
    print(f"regulariser {res}: value achieved / bound = {abs(value - want) / (2.0 ** -24 * abs(want)):.3f}")
    assert abs(value - want) <= 2.0 ** -24 * abs(want)
    bound = 2.0 ** -24 * np.abs(gwant) + 2.0 ** -50 * np.abs(gwant).max()
    err = np.abs(grad - gwant)
    print(f"regulariser {res}: gradient achieved / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all() and np.abs(gwant).min() >= 0 and np.abs(gwant).max() > 0
    with torch.no_grad():
        alone = fh.plane_regularizer(torch.from_numpy(host).to(DEV), cfg, **kw)   # the value alone: no dtable is formed
    assert np.array_equal(bits(alone.cpu().numpy()), bits(outs[0][0]))
    for name in kw:                                            # each weight alone reaches its own planes
        one = {name: 1.0}
        got = float(fh.plane_regularizer(torch.from_numpy(host).to(DEV), cfg, **one))
        ref = float(th.regularizer_torch(torch.from_numpy(host).double(), c, **one))
        assert abs(got - ref) <= 2.0 ** -24 * abs(ref) and (ref > 0 or (name == "smooth_time" and res[3] == 2)), name


# ---- autograd ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd_d4", "multi_d4", "direct_d3"])
def test_autograd_equals_the_raw_calls_and_grid_sample(name):
    import fused_hexplane as fh
    c = fixture(name, "general")
    cfg = config(c["cfg"])
    ref = refs(c)
    cols = th.out_dim(c["cfg"])
    x = torch.from_numpy(c["x"]).to(DEV).requires_grad_(True)
    table = torch.from_numpy(c["table"]).to(DEV).requires_grad_(True)
    g = torch.from_numpy(c["dy"]).to(DEV)
    wide = torch.cat([torch.zeros((len(c["x"]), 3), device=DEV), g, torch.zeros((len(c["x"]), 2), device=DEV)], 1)
    y = fh.hex_plane(x, table, cfg)
    y.backward(wide[:, 3:3 + cols])                     # a column slice of a wider matrix: read in place
    got = dict(y=y.detach().cpu().numpy(), dx=x.grad.cpu().numpy(), dtable=table.grad.cpu().numpy())
    check_general(got, ref, f"{name} autograd")
    # only what is required is formed
    x2 = torch.from_numpy(c["x"]).to(DEV)
    t2 = torch.from_numpy(c["table"]).to(DEV).requires_grad_(True)
    fh.hex_plane(x2, t2, cfg).backward(g)
    assert torch.equal(t2.grad, table.grad)
    y0, dx0, dt0 = fh.hex_plane_and_grads(x2, t2, g, cfg)
    assert torch.equal(y0, y.detach()) and torch.equal(dx0, x.grad) and torch.equal(dt0, table.grad)
    y1, dx1, dt1 = fh.hex_plane_and_grads(x2, t2, g, cfg, want_dx=False, scratch_bytes=512 + int(np.diff(th.offsets(c["cfg"])).max()) * 8)
    assert dx1 is None and torch.equal(dt1, dt0)
    # a K-Planes checkpoint (a list of lists of (1, C, res_b, res_a) planes) loads with the same meaning: F.grid_sample in float32 on the
    # same device, whose own rounding (weights from a float32 position) is 2^-24 res of a cell
    grids = [[p.clone() for p in level] for level in fh.unpack_planes(t2.detach(), cfg)]
    stock = th.hex_plane_torch(x2, fh.pack_planes(grids), c["cfg"])
    scale = float(np.abs(c["table"]).max()) ** len(cfg.planes) * cfg.levels
    assert float((stock - y.detach()).abs().max()) <= 2.0 ** -14 * scale


def test_hexplane_mlp_and_an_adam_step_repeat_bit_for_bit():
    import fused_hexplane as fh
    import fused_mlp as fm
    from fused_params import FusedAdam
    N = 1000
    gen = torch.Generator().manual_seed(5)
    xyz, t = (torch.rand((N, 3), generator=gen) * 2.4 - 1.2).to(DEV), (torch.rand((N, 1), generator=gen) * 2 - 1).to(DEV)
    target = torch.rand((N, 3), generator=gen).to(DEV)
    torch.manual_seed(3)
    field = fh.HexPlane(4, channels=8, base=(8, 8, 8, 5), multires=(1, 2), aabb=((-1.3,) * 3, (1.3,) * 3)).to(DEV)
    mlp = fm.TinyMLP(field.out_dim + 1, 3, hidden=32, hidden_layers=2, output_activation="sigmoid").to(DEV)
    state = [p.detach().clone() for p in [field.table] + list(mlp.parameters())]

    def step():
        params = [field.table] + list(mlp.parameters())
        with torch.no_grad():
            for p, s in zip(params, state):
                p.copy_(s)
                p.grad = None
        loss = ((mlp(torch.cat([field(torch.cat([xyz, t], 1)), t], 1)) - target) ** 2).mean() + field.regularizer(tv_space=1e-2, smooth_time=1e-2, l1_time=1e-3)
        loss.backward()
        grads = [p.grad.clone() for p in params]
        opt = FusedAdam([{"params": [field.table], "lr": 1e-2}, {"params": list(mlp.parameters()), "lr": 1e-3}])
        opt.step()
        return float(loss.detach()), grads, [p.detach().clone() for p in params]

    loss1, g1, p1 = step()
    loss2, g2, p2 = step()
    assert np.isfinite(loss1) and loss1 == loss2
    assert float(g1[0].abs().max()) > 0
    for a, b in zip(g1 + p1, g2 + p2):
        assert torch.equal(a, b)
    for s, p in zip(state, p1):
        assert float((s - p).abs().max()) > 0   # every parameter moved
