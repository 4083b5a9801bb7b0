"""CPU: densification (include/gsr_densify.h, fused_densify.py).  expand(action_codes(...)) of tests/torch_densify.py -- the contract the
kernels are held to -- equals the stock clone, split, prune sequence of the reference row for row: copied values and moments bit for
bit, new moments +0.0, the children's positions within 1e-6 of the row's scale ||xyz|| + ||exp(ls) * n|| (the stock bmm is fp32),
their log-scales within 2e-6 absolute (the stock value carries its fp32 exp and log).  The inputs keep every thresholded quantity
1e-3 relative away from its threshold, which is asserted.  The header compiles as C99 and as C++17 beside gsr.h and when included
twice; every function it declares is exported; the constants fused_densify exports are the header's; the struct layouts are the
header's; every entry point validates its arguments before any device work; the Python surfaces refuse before the kernel library is
loaded.  Nothing here touches a device."""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import torch_densify as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsr_densify.h")
LIB = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "libgsr_hip.so")
INVALID = -1   # GSR_ERR_INVALID_ARGUMENT
NAMES = ["gsr_densify_apply", "gsr_densify_plan", "gsr_densify_scratch_bytes"]


def _lib():
    if not os.path.exists(LIB):
        __graft_entry__.build()
    import fused_densify as fd
    L = fd.bind(ctypes.CDLL(LIB))
    L.gsr_last_error.restype = ctypes.c_char_p
    return L


@pytest.mark.parametrize("screen", (None, ref.SCREEN))
@pytest.mark.parametrize("rest", (0, 15))
@pytest.mark.parametrize("P", (1, 65, 1000))
def test_expanded_action_codes_equal_the_stock_sequence(P, rest, screen):
    import fused_densify as fd
    leaves, moments, grads = ref.make_case(P, rest=rest, seed=P + rest)
    margin = ref.margins(leaves, grads)
    assert margin >= 1e-3, f"a tested quantity lies {margin:.1e} relative from its threshold"
    codes = fd.action_codes(leaves[ref.OPACITY], leaves[ref.SCALING], grads, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, screen)
    assert codes.dtype == torch.uint8 and tuple(codes.shape) == (P,)
    # the noise in the layout of the stock sequence: its split set is every row selected for a split, pruned afterwards or not
    g = torch.nan_to_num(grads.reshape(-1), nan=0.0)
    stock_split = (g >= ref.MAX_GRAD) & (torch.exp(leaves[ref.SCALING]).max(dim=1).values > ref.PERCENT_DENSE * ref.EXTENT)
    S_stock = int(stock_split.sum())
    stock_noise = torch.randn(2 * S_stock, 3, generator=torch.Generator().manual_seed(P))
    kept = (codes == ref.SPLIT)[stock_split]          # of the stock's split rows, those whose children survive
    noise = torch.cat([stock_noise[:S_stock][kept], stock_noise[S_stock:][kept]])
    want, want_moments = ref.stock_densify_and_prune(leaves, moments, grads, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, screen, stock_noise)
    got = ref.expand(leaves, moments, codes, noise)
    K, C, S = got["counts"]
    print(f"P = {P}, rest = {rest}, screen = {screen}: K = {K}, C = {C}, S = {S}, P' = {K + C + 2 * S}, margin {margin:.1e}")
    assert want[0].shape[0] == K + C + 2 * S
    first = K + C
    for k, (a, b) in enumerate(zip(got["leaves"], want)):
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert torch.equal(a[:first], b[:first]), k
        if k not in (ref.XYZ, ref.SCALING):
            assert torch.equal(a, b), k
    if S:
        scale = want[ref.XYZ][first:].double().norm(dim=1) + got["scale"]
        err = (want[ref.XYZ][first:].double() - got["xyz64"]).norm(dim=1) / scale
        ls_err = (want[ref.SCALING][first:].double() - got["leaves"][ref.SCALING][first:].double()).abs()
        print(f"children: xyz {float(err.max()):.1e} relative, log-scales {float(ls_err.max()):.1e} absolute")
        assert float(err.max()) <= 1e-6 and float(ls_err.max()) <= 2e-6
    for k, (a, b) in enumerate(zip(got["moments"], want_moments)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), k
        assert bool((a[0][K:] == 0).all()) and bool((a[1][K:] == 0).all()) and not bool(torch.signbit(a[0][K:]).any()), k
    if P == 1000:   # every code occurs, and the screen-size test removes rows of every kind
        assert all(int((codes == c).sum()) > 0 for c in (ref.KEEP, ref.PRUNE, ref.CLONE, ref.SPLIT))
        if screen:
            plain = fd.action_codes(leaves[ref.OPACITY], leaves[ref.SCALING], grads, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, None)
            assert int(((plain == ref.SPLIT) & (codes == ref.PRUNE)).sum()) > 0 and int(((plain == ref.KEEP) & (codes == ref.PRUNE)).sum()) > 0


def test_explicit_max_radii_prune_a_row_and_what_comes_of_it():
    import fused_densify as fd
    leaves, _, grads = ref.make_case(65, rest=0, seed=3)
    args = (leaves[ref.OPACITY], leaves[ref.SCALING], grads, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT)
    base = fd.action_codes(*args, ref.SCREEN)
    radii = torch.zeros(65)
    radii[::2] = 30.0
    codes = fd.action_codes(*args, ref.SCREEN, max_radii2D=radii)
    assert bool((codes[::2] == ref.PRUNE).all()) and torch.equal(codes[1::2], base[1::2]) and int((base[::2] != ref.PRUNE).sum()) > 0
    assert torch.equal(fd.action_codes(*args, None, max_radii2D=radii), fd.action_codes(*args, None))   # no screen size, no test


def test_reference_rows_follow_the_contract_order():
    action = torch.tensor([ref.CLONE, ref.SPLIT, ref.PRUNE, ref.KEEP, ref.SPLIT, ref.CLONE], dtype=torch.uint8)
    src, K, C, S = ref.source_rows(action)
    assert (K, C, S) == (3, 2, 2) and src.tolist() == [0, 3, 5, 0, 5, 1, 4, 1, 4]


def test_struct_layouts_and_constants_match_the_header():
    import fused_densify as fd
    g, a = fd.DensifyGroup, fd.DensifyArgs
    assert ctypes.sizeof(g) == 56 and g.exp_avg.offset == 8 and g.exp_avg_sq.offset == 16 and g.out_param.offset == 24
    assert g.out_exp_avg.offset == 32 and g.out_exp_avg_sq.offset == 40 and g.row.offset == 48 and g.zero_new.offset == 52
    assert ctypes.sizeof(a) == 80 and a.S.offset == 12 and a.ngroups.offset == 16 and a.xyz_group.offset == 20 and a.rotation_group.offset == 28
    assert a.groups.offset == 32 and a.action.offset == 40 and a.scratch.offset == 48 and a.noise.offset == 56 and a.src_of.offset == 64
    assert a.stream.offset == 72
    hdr = open(HDR).read()
    defines = dict(re.findall(r"#define (GSR_DENSIFY_[A-Z_]+) ([0-9.]+)", hdr))
    assert [int(defines["GSR_DENSIFY_" + n]) for n in ("KEEP", "PRUNE", "CLONE", "SPLIT")] == [fd.KEEP, fd.PRUNE, fd.CLONE, fd.SPLIT] == [0, 1, 2, 3]
    assert int(defines["GSR_DENSIFY_SPLIT_N"]) == fd.SPLIT_N == 2 and int(defines["GSR_DENSIFY_MAX_GROUPS"]) == fd.MAX_GROUPS == 16
    assert int(defines["GSR_DENSIFY_PLAN_ROWS"]) == fd.PLAN_ROWS and int(defines["GSR_DENSIFY_SCAN_THREADS"]) == fd.SCAN_THREADS
    assert float(defines["GSR_DENSIFY_LOG_SHRINK"]) == fd.LOG_SHRINK == ref.LOG_SHRINK
    assert abs(fd.LOG_SHRINK - math.log(1.6)) <= 2.0 ** -53   # the double nearest to log 1.6; math.log takes the double nearest to 1.6
    # the C compiler's view of both structs
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "gsr_densify.h"\nint main(void) { printf("%zu %zu %zu %zu %.17g\\n", '
           "sizeof(gsr_densify_group), sizeof(gsr_densify_args), offsetof(gsr_densify_group, row), offsetof(gsr_densify_args, groups), "
           "GSR_DENSIFY_LOG_SHRINK); return 0; }\n")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "layout.c"), "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), os.path.join(tmp, "layout.c"), "-o", os.path.join(tmp, "layout")],
                       check=True, timeout=120)
        out = subprocess.run([os.path.join(tmp, "layout")], capture_output=True, text=True, check=True, timeout=60).stdout.split()
    assert [int(v) for v in out[:4]] == [56, 80, 48, 32] and float(out[4]) == fd.LOG_SHRINK


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_alongside_the_core_abi(tmp_path, compiler, std, ext):
    src = tmp_path / f"includer.{ext}"
    src.write_text('#include "gsr.h"\n#include "gsr_mcmc.h"\n#include "gsr_densify.h"\n#include "gsr_densify.h"\n'
                   "int gsr_densify_includer(void) { return (int)(sizeof(&gsr_densify_plan) + sizeof(&gsr_densify_apply) + "
                   "sizeof(&gsr_densify_scratch_bytes) + sizeof(gsr_densify_args) + sizeof(gsr_densify_group) + sizeof(&gsr_adam_step)) + "
                   "GSR_DENSIFY_MAX_GROUPS + (GSR_DENSIFY_LOG_SHRINK > 0.47); }\n")
    r = subprocess.run([compiler, std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_every_declared_symbol_is_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr)))
    assert names == NAMES, names
    L = _lib()
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/gsr_densify.h but not exported"


def test_scratch_size_is_zero_for_invalid_sizes_and_grows():
    L = _lib()
    for P in (0, -1, -(1 << 20)):
        assert L.gsr_densify_scratch_bytes(P) == 0, P
    prev = 0
    for P in (1, 1024, 1025, 5000, 1 << 20, 6 << 20, (1 << 31) - 1):
        b = L.gsr_densify_scratch_bytes(P)
        assert b % 16 == 0 and b >= prev and b >= 16 * math.ceil(P / 1024), (P, b)
        prev = b


def test_entry_points_validate_before_any_device_work():
    import fused_densify as fd
    L = _lib()
    one = 4096   # a non-NULL address that must never be dereferenced

    def plan(P=100, action=one, scratch=one, totals=one):
        return L.gsr_densify_plan(P, action, scratch, totals, None)

    for kw in (dict(P=0), dict(P=-3), dict(action=None), dict(scratch=None), dict(totals=None)):
        assert plan(**kw) == INVALID, kw
        assert L.gsr_last_error().startswith(b"gsr_densify_plan:"), (kw, L.gsr_last_error())

    def table(rows=(3, 3, 45, 1, 3, 4), moments=True, **edit):
        t = (fd.DensifyGroup * len(rows))()
        for k, r in enumerate(rows):
            m = one if moments else None
            t[k] = fd.DensifyGroup(one, m, m, one, m, m, r, 0)
        for k, fields in edit.items():
            for f, v in fields.items():
                setattr(t[int(k[1:])], f, v)
        return t

    def apply(groups=table(), ngroups=6, **kw):
        base = dict(P=1000, K=700, C=100, S=100, ngroups=ngroups, xyz_group=0, scale_group=4, rotation_group=5, groups=groups, action=one,
                    scratch=one, noise=one, src_of=one, stream=None)
        base.update(kw)
        return L.gsr_densify_apply(ctypes.byref(fd.DensifyArgs(**base)))

    seventeen = table(rows=(3,) * 17)
    bad = [dict(P=0), dict(P=-1), dict(K=-1), dict(C=-1), dict(S=-1), dict(C=701), dict(K=901, C=0), dict(K=1000, S=1, C=0),
           dict(ngroups=0), dict(groups=seventeen, ngroups=17), dict(groups=None),
           dict(xyz_group=-1), dict(scale_group=-1), dict(rotation_group=-1),                      # needed with S > 0
           dict(xyz_group=6), dict(scale_group=-2), dict(rotation_group=6), dict(S=0, K=900, xyz_group=6), dict(S=0, K=900, rotation_group=-2),
           dict(xyz_group=4), dict(scale_group=0), dict(rotation_group=4),                         # one group twice
           dict(xyz_group=3), dict(xyz_group=5, rotation_group=0), dict(scale_group=3), dict(rotation_group=1),   # rows not 3, 3, 4
           dict(S=0, K=900, xyz_group=2, scale_group=-1, rotation_group=-1),                       # named without a split: still 3 words
           dict(groups=table(g2=dict(row=-1))), dict(groups=table(g0=dict(param=None))), dict(groups=table(g1=dict(out_param=None))),
           dict(groups=table(g1=dict(exp_avg=None))), dict(groups=table(g1=dict(exp_avg_sq=None))),
           dict(groups=table(g1=dict(out_exp_avg=None))), dict(groups=table(g2=dict(out_exp_avg_sq=None))),
           dict(P=47721859, K=100, C=0, S=0),                   # 45 P words exceed 32-bit indexing in the input
           dict(P=40000000, K=30000000, C=30000000, S=0),       # 45 P' do in the output
           dict(action=None), dict(scratch=None), dict(noise=None), dict(src_of=None)]
    for kw in bad:
        assert apply(**kw) == INVALID, kw
        assert L.gsr_last_error().startswith(b"gsr_densify_apply:"), (kw, L.gsr_last_error())
    assert L.gsr_densify_apply(None) == INVALID and L.gsr_last_error().startswith(b"gsr_densify_apply:")
    # P' = 0 is not an error and launches nothing: no output, map or noise is needed; a row of 0 words needs no tensor either
    none = table(**{f"g{k}": dict(out_param=None, out_exp_avg=None, out_exp_avg_sq=None) for k in range(6)})
    assert apply(K=0, C=0, S=0, groups=none, noise=None, src_of=None, xyz_group=-1, scale_group=-1, rotation_group=-1) == 0
    assert apply(K=0, C=0, S=0, groups=table(rows=(3, 3, 0, 1, 3, 4), moments=False, g2=dict(param=None, out_param=None)), noise=None, src_of=None) == 0


def test_python_surfaces_refuse_before_the_library_loads():
    import fused_densify as fd
    from diff_gaussian_rasterization import _C
    from fused_params import FusedAdam
    loaded = _C._lib
    _C._lib = None
    try:
        P = 10
        leaves, moments, grads = ref.make_case(P, rest=2)
        action = torch.zeros(P, dtype=torch.uint8)
        rows = [(p, m, v) for p, (m, v) in zip(leaves, moments)]
        with pytest.raises(RuntimeError, match="no CPU path"):
            fd.densify(rows, action)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fd.prune(rows, action.bool())
        with pytest.raises(RuntimeError, match="bool"):
            fd.prune(rows, action)
        params = [torch.nn.Parameter(p.clone()) for p in leaves]
        opt = FusedAdam([{"params": [p], "lr": 1e-3, "name": n} for p, n in zip(params, fd.LEAF_NAMES)], lr=0.0, eps=1e-15)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fd.densify(opt, action)
        stats = (torch.ones(P), torch.ones(P), torch.zeros(P))
        with pytest.raises(RuntimeError, match="no CPU path"):
            fd.densify_and_prune(opt, stats, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, None)
        with pytest.raises(TypeError, match="three tensors"):
            fd.densify_and_prune(opt, stats[:2], ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, None)
        nameless = FusedAdam([{"params": [p], "lr": 1e-3} for p in params], lr=0.0)
        for call in (lambda: fd.densify(nameless, action), lambda: fd.reset_opacity(nameless)):
            with pytest.raises(RuntimeError, match="named as the reference"):
                call()
        with pytest.raises(ValueError, match="max_opacity"):
            fd.reset_opacity(opt, max_opacity=1.0)
        with pytest.raises(RuntimeError, match="list of"):
            fd.densify([(leaves[0], None)], action)
        with pytest.raises(RuntimeError, match="list of"):
            fd.densify([], action)
        with pytest.raises(RuntimeError, match="pairs"):
            fd.densify(rows, action, extras=[(torch.zeros(P), True, 1)])
        with pytest.raises(RuntimeError, match="at most 16"):
            fd.densify(rows, action, extras=[(torch.zeros(P), False)] * 11)
        with pytest.raises(TypeError):
            fd.densify([(leaves[0], 1.0, None)], action)
        with pytest.raises(TypeError):
            fd.densify(rows, action, extras=[(3, False)])
        with pytest.raises(TypeError):
            fd.densify(rows, [0] * P)
        assert _C._lib is None, "a refusal loaded the kernel library"
        # the remaining refusals come after the device check, which CPU tensors never pass
        _refusals_behind_the_device_check(fd)
        assert _C._lib is None, "a refusal loaded the kernel library"
        # reset_opacity and action_codes are plain torch and run on the CPU
        for p in params:
            opt.state[p] = {"step": 3, "exp_avg": torch.ones_like(p), "exp_avg_sq": torch.ones_like(p)}
        before = params[3].detach().clone()
        assert fd.reset_opacity(opt) is params[3]
        cap = math.log(0.01 / 0.99)
        assert torch.equal(params[3].detach(), before.clamp(max=cap)) and float(params[3].detach().max()) <= cap and bool((before > cap).any())
        assert not bool(opt.state[params[3]]["exp_avg"].any()) and not bool(opt.state[params[3]]["exp_avg_sq"].any())
        assert bool(opt.state[params[0]]["exp_avg"].all()) and opt.state[params[3]]["step"] == 3
    finally:
        _C._lib = loaded


def _refusals_behind_the_device_check(fd):
    """_check_densify on CPU tensors whose `device` attribute says cuda:0: the checks are shape, dtype and stride logic and touch no
    device."""
    P = 10
    leaves, moments, _ = ref.make_case(P, rest=2)
    cuda = torch.device("cuda", 0)

    def dress(t):
        class T(torch.Tensor):
            @property
            def device(self):
                return cuda
        return t.as_subclass(T)

    rows = [(dress(p), dress(m), dress(v)) for p, (m, v) in zip(leaves, moments)]
    action = dress(torch.zeros(P, dtype=torch.uint8))
    check = lambda r=rows, a=action, n=None, e=(), **kw: fd._check_densify(r, a, n, e, **kw)
    assert check()[2:] == ((0, 4, 5), [], P)
    assert check(r=rows[:2], e=[(dress(torch.zeros(P, dtype=torch.int32)), True)])[2] == (0, -1, -1)
    strided = dress(torch.zeros(P, 6)[:, ::2])
    with pytest.raises(RuntimeError, match="contiguous"):
        check(r=rows[:4] + [(rows[4][0], strided, rows[4][2])] + rows[5:])
    with pytest.raises(RuntimeError, match="contiguous"):
        check(e=[(dress(torch.zeros(P, 2)[:, ::2]), False)])
    with pytest.raises(RuntimeError, match="go together"):
        check(r=[(rows[0][0], rows[0][1], None)] + rows[1:])
    with pytest.raises(RuntimeError, match="float32"):
        check(r=[(rows[0][0], dress(torch.zeros(P, 3, dtype=torch.float64)), rows[0][2])] + rows[1:])
    with pytest.raises(RuntimeError, match="of shape"):
        check(r=[(rows[0][0], dress(torch.zeros(P, 4)), rows[0][2])] + rows[1:])
    with pytest.raises(RuntimeError, match="dim 0 = P"):
        check(r=rows[:1] + [(dress(torch.zeros(P + 1, 3)), None, None)] + rows[2:])
    with pytest.raises(RuntimeError, match="dim 0 = P >= 1"):
        check(r=[(dress(torch.zeros(0, 3)), None, None)])
    with pytest.raises(RuntimeError, match="float32 or int32"):
        check(e=[(dress(torch.zeros(P, dtype=torch.int64)), False)])
    with pytest.raises(RuntimeError, match="dim 0 = P"):
        check(e=[(dress(torch.zeros(P + 1)), False)])
    with pytest.raises(RuntimeError, match=r"scaling group must be \(P, 3\)"):
        check(scaling_index=5, rotation_index=None)
    with pytest.raises(RuntimeError, match="three groups"):
        check(xyz_index=4)
    with pytest.raises(RuntimeError, match="uint8"):
        check(a=dress(torch.zeros(P, dtype=torch.int64)))
    with pytest.raises(RuntimeError, match="uint8"):
        check(a=dress(torch.zeros(P + 1, dtype=torch.uint8)))
    with pytest.raises(RuntimeError, match="is on cpu"):
        check(a=torch.zeros(P, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r"\(2 S, 3\)"):
        check(n=dress(torch.zeros(4, 2)))
    with pytest.raises(RuntimeError, match=r"\(2 S, 3\)"):
        check(n=dress(torch.zeros(4, 3, dtype=torch.float64)))
    with pytest.raises(RuntimeError, match="is on cpu"):
        check(n=torch.zeros(4, 3))
