"""CPU: fixed-budget (MCMC) training (include/gsr_mcmc.h, fused_mcmc.py).  The reference of tests/torch_mcmc.py equals, in float64,
the stock sequence a user writes: the noise with the covariance from bmm and an einsum, relocation from bincount(src)[src] + 1 with
the double loop, torch.logit and torch.log, the regulariser through autograd.  The hockey-stick identity that collapses the double
loop holds for n = 1 .. 51.  The header compiles as C99 and as C++17 beside gsr.h and when included twice; every function it declares
is exported; the constants fused_mcmc exports are the header's; the scratch function returns 0 for invalid sizes; every entry point
validates its arguments before any device work; the Python surfaces refuse before the kernel library is loaded.  Nothing here touches
a device."""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import torch_mcmc as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsr_mcmc.h")
LIB = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "libgsr_hip.so")
INVALID = -1   # GSR_ERR_INVALID_ARGUMENT
NAMES = ["gsr_mcmc_noise", "gsr_mcmc_regularizer", "gsr_mcmc_regularizer_scratch_bytes", "gsr_mcmc_relocate"]


def _lib():
    if not os.path.exists(LIB):
        __graft_entry__.build()
    import fused_mcmc as fm
    L = ctypes.CDLL(LIB)
    L.gsr_last_error.restype = ctypes.c_char_p
    L.gsr_mcmc_noise.restype = ctypes.c_int
    L.gsr_mcmc_noise.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_float, ctypes.c_void_p]
    L.gsr_mcmc_relocate.restype = ctypes.c_int
    L.gsr_mcmc_relocate.argtypes = [ctypes.POINTER(fm.RelocateArgs)]
    L.gsr_mcmc_regularizer_scratch_bytes.restype = ctypes.c_size_t
    L.gsr_mcmc_regularizer_scratch_bytes.argtypes = [ctypes.c_int]
    L.gsr_mcmc_regularizer.restype = ctypes.c_int
    L.gsr_mcmc_regularizer.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_float] + [ctypes.c_void_p] * 5
    return L


@pytest.mark.parametrize("P", (1, 63, 1000))
def test_noise_reference_equals_the_stock_sequence_in_float64(P):
    _, _, _, opacity, scaling, rotation = ref.make_leaves(P, seed=P)
    noise = torch.randn(P, 3, generator=torch.Generator().manual_seed(P))
    scaler = 0.8
    d, g, fro = ref.noise_displacement(opacity, scaling, rotation, noise, scaler)
    stock = ref.stock_noise_displacement(opacity, scaling, rotation, noise, scaler, dtype=torch.float64)
    err = float(ref.normalised_noise_error(stock, d, g, fro, noise, scaler).max())
    print(f"P = {P}: reference against the stock sequence in float64, normalised: {err:.1e}; gate {float(g.min()):.1e} .. {float(g.max()):.2f}")
    assert err <= 1e-12
    if P == 1000:   # the gate spans its range: 0.62 for a transparent Gaussian, below fp32's smallest number for an opaque one
        assert float(g.max()) > 0.6 and float(g.min()) < 1e-38


def test_relocation_reference_equals_the_stock_sequence_in_float64():
    P = 40
    leaves = ref.make_leaves(P, rest=0, seed=5, logit_range=6.0)
    g = torch.Generator().manual_seed(6)
    src = torch.cat([torch.full((60,), 7), torch.tensor([3]), torch.randint(20, 30, (9,), generator=g)])
    opac64, scales64 = torch.sigmoid(leaves[3].double()).flatten(), torch.exp(leaves[4].double())
    # gsplat's relocate: ratios from a bincount, compute_relocation's double loop, then logit and log
    ratios = (torch.bincount(src)[src] + 1).clamp(min=1, max=ref.MAX_RATIO)
    for s, n in zip(src.tolist(), ratios.tolist()):
        new_o = 1.0 - (1.0 - opac64[s]) ** (1.0 / n)
        denom = sum(math.comb(i - 1, k) * (-1) ** k * new_o ** (k + 1) / math.sqrt(k + 1) for i in range(1, n + 1) for k in range(i))
        stock_logit = torch.logit(new_o.clamp(min=0.005, max=ref.OPACITY_MAX))
        stock_ls = torch.log(opac64[s] / denom * scales64[s])
        logit, ls = ref.relocation_values(leaves[3][s, 0], leaves[4][s], n, 0.005)
        assert abs(logit - float(stock_logit)) <= 1e-12 * max(1.0, abs(logit)), (s, n)
        assert float((torch.tensor(ls, dtype=torch.float64) - stock_ls).abs().max()) <= 1e-12 * max(1.0, float(stock_ls.abs().max())), (s, n)
    assert int(ratios.max()) == ref.MAX_RATIO and int(ratios.min()) == 2


def test_full_relocation_reference_moves_rows_and_keeps_the_rest():
    P = 12
    leaves = ref.make_leaves(P, rest=2, seed=9, logit_range=4.0)
    moments = [(torch.rand_like(p), torch.rand_like(p)) for p in leaves]
    dst, src = torch.tensor([0, 5, 9]), torch.tensor([3, 3, 7])
    new, mom, exact = ref.relocate(leaves, moments, dst, src, 3, 4, zero_src_moments=True)
    for k in (0, 1, 2, 5):
        assert torch.equal(new[k][dst], leaves[k][src])
    assert torch.equal(new[3][[0, 5]], new[3][[3, 3]]) and torch.equal(new[4][9], new[4][7]) and sorted(exact) == [0, 3, 5, 7, 9]
    rest = [i for i in range(P) if i not in (0, 3, 5, 7, 9)]
    for k in range(6):
        assert torch.equal(new[k][rest], leaves[k][rest])
        assert bool((mom[k][0][[3, 7]] == 0).all()) and bool((mom[k][1][[3, 7]] == 0).all())
        keep = [i for i in range(P) if i not in (3, 7)]
        assert torch.equal(mom[k][0][keep], moments[k][0][keep]) and torch.equal(mom[k][1][keep], moments[k][1][keep])
    # three Gaussians of opacity o' in a row blend like one of opacity o: 1 - (1 - o')^3 = o
    o, o_new = torch.sigmoid(leaves[3][3, 0].double()), torch.sigmoid(torch.tensor(exact[3][0], dtype=torch.float64))
    assert abs(float(1 - (1 - o_new) ** 3) - float(o)) <= 1e-12 or float(o_new) == 0.005


@pytest.mark.parametrize("n", range(1, ref.MAX_RATIO + 1))
def test_hockey_stick_identity_collapses_the_double_loop(n):
    for k in range(n):
        assert sum(math.comb(i - 1, k) for i in range(k + 1, n + 1)) == math.comb(n, k + 1)
    for o_new in (1e-4, 0.03, 0.3, 0.9):
        if (1 + o_new) ** n > 1e4:
            continue   # the alternating sum itself loses more than four digits there, in either form
        a, b = ref.relocation_denominator(o_new, n), ref.collapsed_denominator(o_new, n)
        assert abs(a - b) <= 1e-10 * abs(a), (n, o_new, a, b)


@pytest.mark.parametrize("P", (1, 257))
def test_regulariser_reference_equals_autograd_in_float64(P):
    _, _, _, opacity, scaling, _ = ref.make_leaves(P, seed=P, logit_range=12.0)
    val, d_o, d_s = ref.regularizer(opacity, scaling, 0.01, 0.02)
    l, ls = opacity.double().requires_grad_(True), scaling.double().requires_grad_(True)
    stock = 0.01 * torch.sigmoid(l).mean() + 0.02 * torch.exp(ls).mean()
    g_l, g_s = torch.autograd.grad(stock, (l, ls))
    assert abs(float(val) - float(stock.detach())) <= 1e-12 * float(stock.detach())
    # sigmoid_backward forms y (1 - y): it agrees with sigmoid(l) sigmoid(-l) to what the subtraction leaves
    y = torch.sigmoid(opacity.double())
    assert float(((d_o - g_l).abs() / d_o / (2.0 ** -52 / (1 - y)).clamp(min=1e-12)).max()) <= 4.0
    assert float(((d_s - g_s).abs() / d_s).max()) <= 1e-12


def test_struct_layouts_and_constants_match_the_header():
    import fused_mcmc as fm
    g, a = fm.McmcGroup, fm.RelocateArgs
    assert ctypes.sizeof(g) == 32 and g.exp_avg.offset == 8 and g.exp_avg_sq.offset == 16 and g.row.offset == 24
    assert ctypes.sizeof(a) == 72 and a.zero_src_moments.offset == 20 and a.min_opacity.offset == 24 and a.groups.offset == 32
    assert a.dst.offset == 40 and a.src.offset == 48 and a.counts.offset == 56 and a.stream.offset == 64
    hdr = open(HDR).read()
    defines = dict(re.findall(r"#define (GSR_MCMC_[A-Z_]+) (\d+)", hdr))
    assert int(defines["GSR_MCMC_MAX_RATIO"]) == fm.MAX_RATIO == ref.MAX_RATIO
    assert int(defines["GSR_MCMC_REG_THREADS"]) == fm.REG_THREADS and int(defines["GSR_MCMC_REG_ELEMS_PER_THREAD"]) == fm.REG_ELEMS_PER_THREAD
    core = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert int(re.search(r"#define GSR_ADAM_MAX_GROUPS (\d+)", core).group(1)) == fm.MAX_GROUPS


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_alongside_the_core_abi(tmp_path, compiler, std, ext):
    src = tmp_path / f"includer.{ext}"
    src.write_text('#include "gsr.h"\n#include "gsr_mcmc.h"\n#include "gsr_mcmc.h"\n'
                   "int gsr_mcmc_includer(void) { return (int)(sizeof(&gsr_mcmc_noise) + sizeof(&gsr_mcmc_relocate) + "
                   "sizeof(&gsr_mcmc_regularizer) + sizeof(&gsr_mcmc_regularizer_scratch_bytes) + sizeof(gsr_mcmc_relocate_args) + "
                   "sizeof(gsr_mcmc_group) + sizeof(&gsr_adam_step)) + GSR_MCMC_MAX_RATIO; }\n")
    r = subprocess.run([compiler, std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_every_declared_symbol_is_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr)))
    assert names == NAMES, names
    L = _lib()
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/gsr_mcmc.h but not exported"


def test_scratch_size_is_zero_for_invalid_sizes_and_grows():
    L = _lib()
    for P in (0, -1, -(1 << 20), 1 << 30, (1 << 31) - 1):   # 3 P beyond 32-bit indexing
        assert L.gsr_mcmc_regularizer_scratch_bytes(P) == 0, P
    prev = 0
    for P in (1, 2, 1024, 1025, 5000, 1 << 20, 6 << 20, 715827882):
        b = L.gsr_mcmc_regularizer_scratch_bytes(P)
        assert b > 0 and b % 16 == 0 and b >= prev and b >= 8 * math.ceil(P / 1024), (P, b)
        prev = b


def test_entry_points_validate_before_any_device_work():
    import fused_mcmc as fm
    L = _lib()
    one = 4096   # a non-NULL address that must never be dereferenced

    def noise(P=100, xyz=one, opacity=one, scaling=one, rotation=one, eps=one):
        return L.gsr_mcmc_noise(P, xyz, opacity, scaling, rotation, eps, 0.5, None)

    for kw in (dict(P=0), dict(P=-3), dict(P=1 << 29), dict(xyz=None), dict(opacity=None), dict(scaling=None), dict(rotation=None), dict(eps=None)):
        assert noise(**kw) == INVALID, kw
        assert L.gsr_last_error().startswith(b"gsr_mcmc_noise:"), (kw, L.gsr_last_error())

    def reg(P=100, opacity=one, scaling=one, val=one, scratch=one):
        return L.gsr_mcmc_regularizer(P, opacity, scaling, 0.01, 0.01, val, one, one, scratch, None)

    for kw in (dict(P=0), dict(P=-1), dict(P=1 << 30), dict(opacity=None), dict(scaling=None), dict(val=None), dict(scratch=None)):
        assert reg(**kw) == INVALID, kw
        assert L.gsr_last_error().startswith(b"gsr_mcmc_regularizer:"), (kw, L.gsr_last_error())

    def table(rows=(3, 3, 45, 1, 3, 4), moments=True, **edit):
        t = (fm.McmcGroup * len(rows))()
        for k, r in enumerate(rows):
            t[k] = fm.McmcGroup(one, one if moments else None, one if moments else None, r)
        for k, fields in edit.items():
            for f, v in fields.items():
                setattr(t[int(k[1:])], f, v)
        return t

    def relocate(groups=table(), ngroups=6, **kw):
        base = dict(P=1000, D=10, ngroups=ngroups, opacity_group=3, scale_group=4, zero_src_moments=1, min_opacity=0.005, groups=groups,
                    dst=one, src=one, counts=one, stream=None)
        base.update(kw)
        return L.gsr_mcmc_relocate(ctypes.byref(fm.RelocateArgs(**base)))

    nine = table(rows=(3,) * 9)
    bad = [dict(P=0), dict(P=-1), dict(D=-1), dict(ngroups=0), dict(groups=nine, ngroups=9), dict(groups=None),
           dict(opacity_group=-1), dict(opacity_group=6), dict(scale_group=6), dict(scale_group=-2), dict(opacity_group=4),   # both one group
           dict(opacity_group=0), dict(scale_group=5), dict(scale_group=3, opacity_group=4),                                  # rows not 1 / not 3
           dict(groups=table(g2=dict(row=-1))), dict(groups=table(g0=dict(param=None))), dict(groups=table(g1=dict(exp_avg=None))),
           dict(groups=table(g1=dict(exp_avg_sq=None))),
           dict(min_opacity=0.0), dict(min_opacity=1.0), dict(min_opacity=-0.5), dict(min_opacity=float("nan")),
           dict(P=1 << 30),                                     # 3 P floats exceed 32-bit indexing
           dict(P=47721859),                                    # 45 P does
           dict(D=1 << 27),                                     # more workgroups than one launch takes
           dict(dst=None), dict(src=None), dict(counts=None)]
    for kw in bad:
        assert relocate(**kw) == INVALID, kw
        assert L.gsr_last_error().startswith(b"gsr_mcmc_relocate:"), (kw, L.gsr_last_error())
    assert L.gsr_mcmc_relocate(None) == INVALID and L.gsr_last_error().startswith(b"gsr_mcmc_relocate:")
    # D = 0 is not an error and launches nothing: no pointer is needed; a row of 0 floats needs no tensor either
    assert relocate(D=0, dst=None, src=None, counts=None) == 0
    assert relocate(D=0, groups=table(rows=(3, 3, 0, 1, 3, 4), moments=False, g2=dict(param=None))) == 0


def test_python_surfaces_refuse_before_the_library_loads():
    import fused_mcmc as fm
    from diff_gaussian_rasterization import _C
    from fused_params import FusedAdam
    loaded = _C._lib
    _C._lib = None
    try:
        P = 10
        xyz, dc, fr, opacity, scaling, rotation = ref.make_leaves(P, rest=2)
        noise = torch.randn(P, 3)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fm.inject_noise(xyz, opacity, scaling, rotation, 0.5, noise=noise)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fm.inject_noise(xyz, opacity, scaling, rotation, 0.5)
        with pytest.raises(RuntimeError, match="float32"):
            fm.inject_noise(xyz.double(), opacity, scaling, rotation, 0.5)
        with pytest.raises(RuntimeError, match="float32"):
            fm.inject_noise(xyz, opacity, scaling.half(), rotation, 0.5)
        for kw in (dict(xyz=xyz[:, :2]), dict(opacity=opacity[:, 0]), dict(opacity=opacity[:5]), dict(scaling=rotation), dict(rotation=scaling),
                   dict(noise=noise[1:]), dict(xyz=xyz[:0], opacity=opacity[:0], scaling=scaling[:0], rotation=rotation[:0])):
            args = dict(xyz=xyz, opacity=opacity, scaling=scaling, rotation=rotation, noise=None)
            args.update(kw)
            with pytest.raises(RuntimeError, match=r"must be \(P, \d\)"):
                fm.inject_noise(args["xyz"], args["opacity"], args["scaling"], args["rotation"], 0.5, noise=args["noise"])
        with pytest.raises(TypeError):
            fm.inject_noise([[0.0] * 3], opacity, scaling, rotation, 0.5)

        for fn in (fm.regularizer, fm.regularizer_and_grads):
            with pytest.raises(RuntimeError, match="no CPU path"):
                fn(opacity, scaling)
            with pytest.raises(RuntimeError, match="float32"):
                fn(opacity.double(), scaling.double())
            for o, s in ((opacity[:, 0], scaling), (opacity, scaling[:, :2]), (opacity[:4], scaling), (opacity, rotation)):
                with pytest.raises(RuntimeError, match=r"must be \(P, \d\)"):
                    fn(o, s)
            with pytest.raises(TypeError):
                fn(0.5, scaling)

        dst, src = torch.tensor([0, 1]), torch.tensor([4, 4])
        rows = [(p, torch.zeros_like(p), torch.zeros_like(p)) for p in (xyz, dc, fr, opacity, scaling, rotation)]
        with pytest.raises(RuntimeError, match="no CPU path"):
            fm.relocate(rows, dst, src)
        params = [torch.nn.Parameter(p.clone()) for p in (xyz, dc, fr, opacity, scaling, rotation)]
        opt = FusedAdam([{"params": [p], "lr": 1e-3, "name": n} for p, n in zip(params, fm.LEAF_NAMES)], lr=0.0, eps=1e-15)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fm.relocate(opt, dst, src)
        for helper in (lambda: fm.relocate_dead(opt), lambda: fm.add_new(opt, 100)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                helper()
        nameless = FusedAdam([{"params": [p], "lr": 1e-3} for p in params], lr=0.0)
        with pytest.raises(RuntimeError, match="named 'opacity'"):
            fm.relocate(nameless, dst, src)
        with pytest.raises(RuntimeError, match="groups"):
            fm.relocate(rows * 2, dst, src)
        with pytest.raises(RuntimeError, match="list of"):
            fm.relocate([(xyz, None)], dst, src)
        with pytest.raises(RuntimeError, match="two of the"):
            fm.relocate(rows, dst, src, opacity_index=4)
        assert _C._lib is None, "a refusal loaded the kernel library"
        # the remaining refusals come after the device check, which CPU tensors never pass
        _refusals_behind_the_device_check(fm)
        assert _C._lib is None, "a refusal loaded the kernel library"
    finally:
        _C._lib = loaded


def _refusals_behind_the_device_check(fm):
    """_check_relocate on CPU tensors whose `device` attribute says cuda:0: the checks are shape, dtype and stride logic and touch no
    device."""
    P = 10
    leaves = ref.make_leaves(P, rest=2)
    cuda = torch.device("cuda", 0)

    def dress(t):
        class T(torch.Tensor):
            @property
            def device(self):
                return cuda
        return t.as_subclass(T)

    rows = [(dress(p), dress(torch.zeros_like(p)), dress(torch.zeros_like(p))) for p in leaves]
    dst, src = dress(torch.tensor([0, 1])), dress(torch.tensor([4, 4]))
    check = lambda r=rows, d=dst, s=src, m=0.005, io=3, isc=4: fm._check_relocate(r, d, s, m, io, isc)
    assert check()[3:] == (P, 2)
    strided = dress(torch.zeros(P, 6)[:, ::2])
    with pytest.raises(RuntimeError, match="contiguous"):
        check(r=rows[:4] + [(rows[4][0], strided, rows[4][2])] + rows[5:])
    with pytest.raises(RuntimeError, match="contiguous"):
        check(r=[(dress(torch.zeros(P, 6)[:, ::2]), None, None)] + rows[1:])
    with pytest.raises(RuntimeError, match="go together"):
        check(r=[(rows[0][0], rows[0][1], None)] + rows[1:])
    with pytest.raises(RuntimeError, match="float32"):
        check(r=[(rows[0][0], dress(torch.zeros(P, 3, dtype=torch.float64)), rows[0][2])] + rows[1:])
    with pytest.raises(RuntimeError, match="of shape"):
        check(r=[(rows[0][0], dress(torch.zeros(P, 4)), rows[0][2])] + rows[1:])
    with pytest.raises(RuntimeError, match="dim 0 = P"):
        check(r=[(dress(torch.zeros(P + 1, 3)), None, None)] + rows[1:])
    with pytest.raises(RuntimeError, match=r"\(P, 1\)"):
        check(io=0, isc=4)
    with pytest.raises(RuntimeError, match="int64"):
        check(d=dress(torch.tensor([0, 1], dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="int64"):
        check(s=dress(torch.tensor([[4, 4]])))
    with pytest.raises(RuntimeError, match="one length"):
        check(s=dress(torch.tensor([4])))
    with pytest.raises(RuntimeError, match="is on cpu"):
        check(d=torch.tensor([0, 1]))
    for m in (0.0, 1.0, -1.0):
        with pytest.raises(ValueError, match="min_opacity"):
            check(m=m)
