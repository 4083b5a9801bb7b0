"""GPU: the fused MLP (include/gsr_mlp.h, csrc/mlp.hip, fused_mlp) against the references of tests/torch_mlp.py, whose fixtures
tests/test_mlp_cpu.py validates.  Raw calls write into buffers with canary elements behind and between the rows of every output.

Integer cases are exact (array_equal): they pin the lane map, the padding in k and in the last tile, the layer-to-layer transposes and
the completeness of the dW reduction across waves, tiles and workgroups.  General cases: every decided element of z_M and of dx
equals the float32 chain emulation bit for bit; with an output activation or the encoding the value lies within
2^-24 |ref| + 2^-40 (moduli) of the double evaluation on the emulated z_M; dW and db lie within gamma_n sum |dz a| of the emulated
terms' float64 sum; and independently everything lies within torch_mlp.bars() of the float64 rule on the rows that are not fragile."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
import torch_mlp as tm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CANARY = 12345.0
ACT = {"none": 0, "relu": 1, "sigmoid": 2, "tanh": 3}
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


def raw(case, *, act="relu", outa="none", L=0, xl="rows", yl="rows", pad=0, want=("dx", "dW", "db"), wg=0, backward=True, N=None, skip=()):
    """The two entry points on a fixture -> dict(y, dx, dW, db) of numpy arrays in (N, width) orientation; what is not wanted is None.
    skip: pairs ("dW" or "db", layer index) whose single entry of the pointer array is NULL"""
    import fused_mlp as fm
    x, Ws, bs, dy = case["x"], case["Ws"], case["bs"], case["dy"]
    N = x.shape[0] if N is None else N
    x, dy = x[:N], dy[:N]
    D, M, dM = x.shape[1], len(Ws), Ws[-1].shape[0]
    d = fm.MlpDesc(N=N, M=M, D=D, L=L, hidden_activation=ACT[act], output_activation=ACT[outa], x_layout=int(xl == "planes"),
                   y_layout=int(yl == "planes"), max_workgroups=wg)
    d.widths[0] = D * (1 + 2 * L)
    for l, W in enumerate(Ws):
        d.widths[l + 1] = W.shape[0]
    io = lambda a, planes: Guarded(a.shape[1], a.shape[0], pad, a.T) if planes else Guarded(a.shape[0], a.shape[1], pad, a)
    gx, gdy = io(x, xl == "planes"), io(dy, yl == "planes")
    gy = io(np.full((N, dM), CANARY), yl == "planes")
    gdx = io(np.full((N, D), CANARY), xl == "planes")
    d.x_stride, d.dx_stride, d.y_stride, d.dy_stride = gx.stride, gdx.stride, gy.stride, gdy.stride
    if N == 0:
        d.x_stride = d.dx_stride = D
        d.y_stride = d.dy_stride = dM
    tW = [torch.from_numpy(W).to(DEV) for W in Ws]
    tb = [None if bs is None else torch.from_numpy(b).to(DEV) for b in (bs or [None] * M)]
    gW = [Guarded(W.shape[0], W.shape[1]) for W in Ws]
    gb = [Guarded(1, W.shape[0]) for W in Ws]
    scratch = torch.empty((max(16, fm._lib().gsr_mlp_scratch_bytes(ctypes.byref(d))),), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    fm._run("gsr_mlp_forward", ctypes.byref(d), gx.ptr(), fm._pointers(tW), fm._pointers(tb), gy.ptr(), scratch.data_ptr(), stream)
    out = dict(y=gy.numpy().T if yl == "planes" else gy.numpy(), dx=None, dW=None, db=None)
    if backward:
        ptrs = lambda gs, kind: (ctypes.c_void_p * M)(*[g.ptr() if kind in want and (kind, l) not in skip else None for l, g in enumerate(gs)])
        fm._run("gsr_mlp_backward", ctypes.byref(d), gx.ptr(), fm._pointers(tW), fm._pointers(tb), gdy.ptr(), gdx.ptr() if "dx" in want else None,
                ptrs(gW, "dW"), ptrs(gb, "db"), scratch.data_ptr(), stream)
        torch.cuda.synchronize()
        dxv = gdx.numpy()
        out["dx"] = (dxv.T if xl == "planes" else dxv) if "dx" in want else None
        if "dx" not in want:
            assert (dxv == CANARY).all()
        left = lambda g: None if (g.numpy() == CANARY).all() else "written"
        out["dW"] = [g.numpy() if "dW" in want and ("dW", l) not in skip else left(g) for l, g in enumerate(gW)]
        out["db"] = [g.numpy()[0] if "db" in want and ("db", l) not in skip else left(g) for l, g in enumerate(gb)]
    return out


def exact(case, act="relu"):
    """The float64 rule on an integer fixture, where it is exact -> dict(y, dx, dW, db) float32"""
    key = id(case)
    if key not in _cache:
        x, Ws, bs, dy = tm.t64(case)
        y = tm.mlp_ref(x, Ws, bs, act)
        dx, dW, db = tm.backward_ref(x, Ws, bs, dy, act)
        f = lambda t: t.numpy().astype(np.float32)
        _cache[key] = (case, dict(y=f(y), dx=f(dx), dW=[f(t) for t in dW], db=[f(t) for t in db]))
    return _cache[key][1]


def fixture(name, asymmetric=False):
    key = (name, asymmetric)
    if key not in _cache:
        _cache[key] = tm.integer_fixture(name, asymmetric) if name in tm.INTEGER_SHAPES else tm.general_fixture(name)
    return _cache[key]


def assert_exact(got, ref, what):
    assert np.array_equal(got["y"], ref["y"]), (what, "y")
    assert np.array_equal(got["dx"], ref["dx"]), (what, "dx")
    for l, (a, b) in enumerate(zip(got["dW"], ref["dW"])):
        assert np.array_equal(a, b), (what, "dW", l, np.argwhere(a != b)[:4])
    for l, (a, b) in enumerate(zip(got["db"], ref["db"])):
        assert np.array_equal(a, b), (what, "db", l)


# ---- integer cases: exact ------------------------------------------------------------------------------------------------------------
LAYOUTS = [("rows", "rows", 0), ("planes", "planes", 0), ("rows", "planes", 3), ("planes", "rows", 5), ("rows", "rows", 7)]


@pytest.mark.parametrize("asymmetric", [False, True])
@pytest.mark.parametrize("name", sorted(tm.INTEGER_SHAPES))
def test_integer_cases_are_exact(name, asymmetric):
    c = fixture(name, asymmetric)
    xl, yl, pad = LAYOUTS[(sorted(tm.INTEGER_SHAPES).index(name) + asymmetric) % len(LAYOUTS)]
    assert_exact(raw(c, xl=xl, yl=yl, pad=pad), exact(c), (name, xl, yl, pad))


@pytest.mark.parametrize("xl,yl,pad", LAYOUTS)
def test_every_layout_on_both_sides(xl, yl, pad):
    c = fixture("m3_c", True)
    assert_exact(raw(c, xl=xl, yl=yl, pad=pad), exact(c), (xl, yl, pad))


def test_no_hidden_activation_and_no_bias():
    c = tm.integer_case(100, [5, 33, 4], seed=77, fan_in=3, bias=False)
    x, Ws, bs, dy = tm.t64(c)
    dx, dW, db = tm.backward_ref(x, Ws, None, dy, "none")
    got = raw(c, act="none")
    f = lambda t: t.numpy().astype(np.float32)
    assert_exact(got, dict(y=f(tm.mlp_ref(x, Ws, None, "none")), dx=f(dx), dW=[f(t) for t in dW], db=[f(t) for t in db]), "plain")


@pytest.mark.parametrize("wg", [1, 2, 3])
def test_max_workgroups_integer(wg):
    """Several trips of the persistent loop and several partials at N = 1000: the same exact answers"""
    for name in ("m2_d", "m5_b"):
        c = fixture(name)
        assert_exact(raw(c, wg=wg), exact(c), (name, wg))


# ---- general cases -------------------------------------------------------------------------------------------------------------------
def _emulated(name):
    key = ("em", name)
    if key not in _cache:
        c = fixture(name)
        _cache[key] = tm.emulate(c["x"], c["Ws"], c["bs"], c["dy"])
    return _cache[key]


def _float64(name, outa="none"):
    key = ("f64", name, outa)
    if key not in _cache:
        x, Ws, bs, dy = tm.t64(fixture(name))
        dx, dW, db = tm.backward_ref(x, Ws, bs, dy, "relu", outa)
        _cache[key] = dict(y=tm.mlp_ref(x, Ws, bs, "relu", outa).numpy(), dx=dx.numpy(), dW=[t.numpy() for t in dW], db=[t.numpy() for t in db],
                           bars=tm.bars(x, Ws, bs, dy, "relu", outa))
    return _cache[key]


def _check_sums(got, em, rows, G):
    """dW and db against the float64 sum of the emulated float32 terms, bar gamma_n sum |dz a| with n the additions into the element"""
    n = int(rows.sum()) + G
    worst = 0.0
    for l in range(len(em["dz"])):
        dz, a = em["dz"][l][rows].astype(np.float64), em["a"][l][rows].astype(np.float64)
        ref, bar = dz.T @ a, tm.gamma(n) * (np.abs(dz).T @ np.abs(a))
        err = np.abs(got["dW"][l] - ref)
        assert (err <= bar).all(), ("dW", l, float((err - bar).max()))
        rb, bb = dz.sum(0), tm.gamma(n) * np.abs(dz).sum(0)
        assert (np.abs(got["db"][l] - rb) <= bb).all(), ("db", l)
        worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
    return worst


@pytest.mark.parametrize("name", sorted(tm.GENERAL_SHAPES))
def test_general_cases_equal_the_float32_chain(name):
    c, em = fixture(name), _emulated(name)
    got = raw(c, xl="planes" if name == "g_odd" else "rows", yl="planes" if name == "g_64x2" else "rows")
    ok = ~em["undecided"]
    assert ok.mean() >= 0.999
    assert np.array_equal(got["y"][ok].view(np.uint32), em["z"][ok].view(np.uint32)), "z_M differs from the fmaf chain"
    assert np.array_equal(got["dx"][ok].view(np.uint32), em["dx"][ok].view(np.uint32)), "dx differs from the fmaf chain"
    if not ok.all():   # undecided rows are left out of the sums on both sides
        got = raw({k: (v[ok] if k in ("x", "dy") else v) for k, v in c.items()})
    worst = _check_sums(got, em, ok, 256)
    print(f"{name}: dW achieved / bar = {worst:.3f}")


@pytest.mark.parametrize("outa", ["none", "sigmoid", "tanh"])
@pytest.mark.parametrize("name", sorted(tm.GENERAL_SHAPES))
def test_general_cases_against_float64(name, outa):
    c, ref = fixture(name), _float64(name, outa)
    got = raw(c, outa=outa)
    b = ref["bars"]
    keep = ~b["fragile"].numpy()
    assert keep.mean() >= 0.99
    if outa != "none":   # the output activation alone: the double evaluation on the emulated z_M, rounded once
        z = _emulated(name)["z"].astype(np.float64)
        want = 1 / (1 + np.exp(-z)) if outa == "sigmoid" else np.tanh(z)
        assert (np.abs(got["y"] - want) <= 2.0 ** -24 * np.abs(want) + 2.0 ** -40).all()
    ratio = {}
    for k in ("y", "dx"):
        err, bar = np.abs(got[k] - ref[k]), b[k].numpy()
        rows = keep if k == "dx" else np.ones_like(keep)
        ratio[k] = float((err[rows] / np.maximum(bar[rows], 1e-300)).max())
        assert (err[rows] <= bar[rows]).all(), (k, ratio[k])
    if keep.all():
        for k in ("dW", "db"):
            for l in range(len(ref[k])):
                err, bar = np.abs(got[k][l] - ref[k][l]), b[k][l].numpy()
                ratio[f"{k}{l}"] = float((err / np.maximum(bar, 1e-300)).max())
                assert (err <= bar).all(), (k, l, ratio[f"{k}{l}"])
    else:   # the fragile rows are left out on both sides
        cut = {kk: (v[keep] if kk in ("x", "dy") else v) for kk, v in c.items()}
        x, Ws, bs, dy = tm.t64(cut)
        _, dW, db = tm.backward_ref(x, Ws, bs, dy, "relu", outa)
        bc = tm.bars(x, Ws, bs, dy, "relu", outa)
        gc = raw(cut, outa=outa)
        for k, r in (("dW", dW), ("db", db)):
            for l in range(len(r)):
                err, bar = np.abs(gc[k][l] - r[l].numpy()), bc[k][l].numpy()
                ratio[f"{k}{l}"] = float((err / np.maximum(bar, 1e-300)).max())
                assert (err <= bar).all(), (k, l, ratio[f"{k}{l}"])
    print(f"{name} {outa}: achieved / bar = " + ", ".join(f"{k} {v:.3f}" for k, v in ratio.items()))


@pytest.mark.parametrize("L,D", [(1, 5), (10, 4)])
def test_frequency_encoding(L, D):
    """D raw columns, L octaves: z_M within 2^-24 |ref| + 2^-40 (moduli) of the chain on the encoded row float32(sin / cos in double);
    y, dx, dW and db within the float64 bars"""
    c = tm.encoded_fixture(L, D)
    got = raw(c, L=L, xl="planes")
    x = c["x"]
    enc = [x] + [f((x * np.float32(2.0 ** j)).astype(np.float64)).astype(np.float32) for j in range(L) for f in (np.sin, np.cos)]
    em = tm.emulate(np.concatenate(enc, 1), c["Ws"], c["bs"])
    x64, Ws, bs, dy = tm.t64(c)
    _, zabs = tm.mlp_ref(x64, Ws, bs, L=L, absolute=True, layers=True)
    ok = ~em["undecided"]
    assert (np.abs(got["y"] - em["z"])[ok] <= (2.0 ** -24 * np.abs(em["z"]) + 2.0 ** -40 * zabs[-1].numpy())[ok]).all()
    b = tm.bars(x64, Ws, bs, dy, L=L)
    keep = ~b["fragile"].numpy()
    assert keep.mean() >= 0.99
    dx, dW, db = tm.backward_ref(x64, Ws, bs, dy, L=L)
    assert (np.abs(got["y"] - tm.mlp_ref(x64, Ws, bs, L=L).numpy()) <= b["y"].numpy()).all()
    r = np.abs(got["dx"] - dx.numpy())[keep] / b["dx"].numpy()[keep]
    assert (r <= 1).all(), float(r.max())
    print(f"L = {L}: dx achieved / bar = {float(r.max()):.3f}")
    if keep.all():
        for l in range(3):
            assert (np.abs(got["dW"][l] - dW[l].numpy()) <= b["dW"][l].numpy()).all(), l
            assert (np.abs(got["db"][l] - db[l].numpy()) <= b["db"][l].numpy()).all(), l


@pytest.mark.parametrize("wg", [1, 2, 3])
def test_max_workgroups_general(wg):
    c, em = fixture("g_64x2"), _emulated("g_64x2")
    ok = ~em["undecided"]
    got = raw({k: (v[ok] if k in ("x", "dy") else v) for k, v in c.items()}, wg=wg)
    assert _same_bits(got["y"], em["z"][ok]) and _same_bits(got["dx"], em["dx"][ok])
    _check_sums(got, em, ok, wg)


# ---- further cases -------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    if a is None or b is None:
        return a is b
    if isinstance(a, list):
        return all(_same_bits(p, q) for p, q in zip(a, b))
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_two_calls_give_equal_bits_and_outputs_are_optional():
    c = fixture("g_odd")
    first, again = raw(c, outa="tanh"), raw(c, outa="tanh")
    for k in ("y", "dx", "dW", "db"):
        assert _same_bits(first[k], again[k]), k
    for drop in ("dx", "dW", "db"):
        part = raw(c, outa="tanh", want=tuple(k for k in ("dx", "dW", "db") if k != drop))
        for k in ("dx", "dW", "db"):
            if k == drop:
                assert part[k] is None or all(v is None for v in part[k]), (drop, "was written")
            else:
                assert _same_bits(first[k], part[k]), (drop, k)
    # single entries of the pointer arrays: a frozen layer among trained ones
    part = raw(c, outa="tanh", skip=(("dW", 1), ("db", 0), ("db", 3)))
    assert _same_bits(first["dx"], part["dx"])
    for k, gone in (("dW", (1,)), ("db", (0, 3))):
        for l in range(4):
            assert (part[k][l] is None) if l in gone else _same_bits(first[k][l], part[k][l]), (k, l)


def test_no_rows():
    c = fixture("m2_b")
    got = raw(c, N=0)
    assert got["y"].shape == (0, 3) and got["dx"].shape == (0, 31)
    assert all((w == 0).all() for w in got["dW"]) and all((b == 0).all() for b in got["db"])
    import fused_mlp as fm
    y, dx, dW, db = fm.mlp_and_grads(torch.zeros((0, 31), device=DEV), [torch.from_numpy(W).to(DEV) for W in c["Ws"]], None,
                                     torch.zeros((0, 3), device=DEV))
    assert y.shape == (0, 3) and dx.shape == (0, 31) and all(float(w.abs().sum()) == 0 for w in dW + db)


def test_nan_and_inf_rows_stay_in_their_rows():
    c = fixture("g_scaffold")
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    bad["x"][5, 3], bad["x"][40, 0], bad["x"][255, 34], bad["x"][256, 1] = np.nan, np.inf, -np.inf, np.nan
    rows = np.array([5, 40, 255, 256])
    clean, got = raw(c, want=("dx",)), raw(bad, want=("dx",))
    others = np.ones(257, bool)
    others[rows] = False
    assert _same_bits(clean["y"][others], got["y"][others]) and _same_bits(clean["dx"][others], got["dx"][others])
    with np.errstate(invalid="ignore"):
        em = tm.emulate(bad["x"][rows], c["Ws"], c["bs"], c["dy"][rows])
    assert np.isnan(em["z"]).any()
    np.testing.assert_array_equal(got["y"][rows], em["z"])      # NaN where the rule says NaN, the same values elsewhere
    np.testing.assert_array_equal(got["dx"][rows], em["dx"])


# ---- surface ---------------------------------------------------------------------------------------------------------------------------
def test_tiny_mlp_against_its_own_sequential():
    import fused_mlp as fm
    torch.manual_seed(3)
    for kw in (dict(in_dim=32, out_dim=3, hidden=64, hidden_layers=2, output_activation="sigmoid"),
               dict(in_dim=4, out_dim=3, hidden=64, hidden_layers=2, frequencies=10), dict(in_dim=35, out_dim=70, hidden=32, hidden_layers=1, output_activation="tanh")):
        m = fm.TinyMLP(**kw).to(DEV)
        seq = m.to_sequential().double()
        x = (torch.randn(500, kw["in_dim"], device=DEV) * (0.01 if kw.get("frequencies") else 1.0)).requires_grad_(True)
        g = torch.randn(500, kw["out_dim"], device=DEV)
        (m(x) * g).sum().backward()
        x64 = x.detach().double().requires_grad_(True)
        y64 = seq(x64)
        (y64 * g.double()).sum().backward()
        # the raw calls' own bars (torch_mlp.bars): y everywhere, dx on the rows that are not fragile, dW and db where no row is
        # (with fragile rows in the sums, 1e-4 of the largest element: this is the surface's test, the raw calls carry the bars)
        cpu64 = lambda t: t.detach().double().cpu()
        b = tm.bars(cpu64(x), [cpu64(w) for w in m.weights], [cpu64(v) for v in m.biases], cpu64(g), "relu",
                    kw.get("output_activation", "none"), kw.get("frequencies", 0))
        keep = ~b["fragile"]
        assert float(keep.double().mean()) >= 0.97
        assert bool(((cpu64(m(x)) - cpu64(y64)).abs() <= b["y"]).all())
        assert bool(((cpu64(x.grad) - cpu64(x64.grad)).abs()[keep] <= b["dx"][keep]).all())
        lin = [mod for mod in seq if isinstance(mod, torch.nn.Linear)]
        for l, mod in enumerate(lin):
            for got, ref, bar in ((m.weights[l].grad, mod.weight.grad, b["dW"][l]), (m.biases[l].grad, mod.bias.grad, b["db"][l])):
                err = (cpu64(got) - cpu64(ref)).abs()
                assert bool((err <= bar).all()) if bool(keep.all()) else float(err.max()) <= 1e-4 * max(1.0, float(ref.abs().max())), l
        # a frozen decoder and an input without a gradient: nothing is formed for them
        for p in m.parameters():
            p.requires_grad_(False)
            p.grad = None
        x2 = x.detach().clone().requires_grad_(True)
        (m(x2) * g).sum().backward()
        assert torch.equal(x2.grad, x.grad) and all(p.grad is None for p in m.parameters())


def test_decode_feature_map_and_an_adam_step():
    import fused_mlp as fm
    import gsr_scene
    import util
    from diff_gaussian_rasterization import GaussianRasterizer
    from fused_params import FusedAdam
    scene, cam, K = gsr_scene.make_scene(2000, -3.0, sh_degree=1, seed=33), gsr_scene.make_camera(64, 48), 5
    H, W = cam.image_height, cam.image_width
    torch.manual_seed(9)
    dec = fm.TinyMLP(K, 3, hidden=32, hidden_layers=2, output_activation="sigmoid").to(DEV)
    feats = torch.randn(2000, K, generator=torch.Generator().manual_seed(41))
    g = torch.randn(3, H, W, generator=torch.Generator().manual_seed(43)).to(DEV)

    def render():
        t = {k: getattr(scene, k).to(DEV).clone().requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
        t["means2D"] = torch.zeros(scene.means3D.shape, device=DEV, requires_grad=True)
        f = feats.to(DEV).clone().requires_grad_(True)
        return GaussianRasterizer(util.hip_settings(scene, cam, 1, DEV))(**t, features=f)[-1], f, t

    fmap, f, t = render()
    assert fmap.shape == (K, H, W)
    rgb = fm.decode_feature_map(fmap, dec)
    assert rgb.shape == (3, H, W)
    Ws, bs = [w.detach() for w in dec.weights], [b.detach() for b in dec.biases]
    y, dx, dW, db = fm.mlp_and_grads(fmap.detach().reshape(K, H * W), Ws, bs, g.reshape(3, H * W), output_activation="sigmoid", layout="planes")
    assert torch.equal(rgb.detach().reshape(3, H * W), y)                     # the planes raw call, bit for bit
    (rgb * g).sum().backward()
    for l in range(3):
        assert torch.equal(dec.weights[l].grad, dW[l]) and torch.equal(dec.biases[l].grad, db[l]), l
    fmap2, f2, t2 = render()
    fmap2.backward(dx.reshape(K, H, W))                                         # the raw backward fed by hand
    assert float(f.grad.abs().max()) > 0 and torch.equal(f.grad, f2.grad)
    assert float(t["means3D"].grad.abs().max()) > 0 and torch.equal(t["means3D"].grad, t2["means3D"].grad)
    # one Adam step over the module's parameters as one group, against torch.optim.Adam on copies
    params = list(dec.parameters())
    before = [p.detach().clone() for p in params]
    twins = [p.detach().clone().requires_grad_(True) for p in params]
    for p, q in zip(params, twins):
        q.grad = p.grad.clone()
    FusedAdam(params, lr=1e-2).step()
    torch.optim.Adam(twins, lr=1e-2).step()
    for p, q in zip(params, twins):
        assert float((p.detach() - q.detach()).abs().max()) <= 1e-6
    assert all(float((p.detach() - b).abs().max()) > 0 for p, b in zip(params, before))
