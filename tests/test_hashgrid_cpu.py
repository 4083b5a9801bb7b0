"""CPU: the references of the hash-grid encoding against each other and against exact rationals, the fixtures' promises, the level table
against the library's host code, the C ABI's refusals, every Python refusal, and hashgrid.hip's resource usage.  No GPU is touched."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import torch_hashgrid as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsr_hashgrid.h")
CSRC = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "csrc")
LIB = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "libgsr_hip.so")
NAMES = ["gsr_hashgrid_backward", "gsr_hashgrid_forward", "gsr_hashgrid_layout", "gsr_hashgrid_level_path", "gsr_hashgrid_level_scale",
         "gsr_hashgrid_scratch_bytes"]
DEFAULT = (3, 16, 2, 19, 16, 2.0)


def _lib():
    if not os.path.exists(LIB):
        __graft_entry__.build()
    import fused_hashgrid
    return fused_hashgrid._lib()


def _desc(cfg=(3, 3, 2, 12, 8, 2.0), N=10, xs=None, ys=None, dys=None, dxs=None):
    import fused_hashgrid as fh
    D, L, F, T, base, pls = cfg
    d = fh.HashGridDesc(N=N, D=D, L=L, F=F, base_resolution=base, per_level_scale=pls, log2_hashmap_size=T)
    d.x_stride = D if xs is None else xs
    d.y_stride = L * F if ys is None else ys
    d.dy_stride = L * F if dys is None else dys
    d.dx_stride = D if dxs is None else dxs
    return d


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_is_c99(tmp_path):
    src = tmp_path / "use_hashgrid.c"
    src.write_text('#include "gsr_hashgrid.h"\n#include "gsr_hashgrid.h"\n'
                   "int use(void) { gsr_hashgrid_desc d; d.N = 0; return (int)(sizeof(&gsr_hashgrid_forward) + sizeof(&gsr_hashgrid_backward) + sizeof d) + "
                   "GSR_HASHGRID_MAX_LEVELS + GSR_HASHGRID_PATH_LDS + GSR_HASHGRID_LDS_BYTES + d.N; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "use_hashgrid.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_library_exports_the_names_of_the_header():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr))) == NAMES
    L = _lib()
    for n in NAMES:
        assert hasattr(L, n), n


def test_the_record_is_the_headers():
    import fused_hashgrid as fh
    assert ctypes.sizeof(fh.HashGridDesc) == 4 * 7 + 4 + 8 * 4   # seven 4-byte fields, padding, four strides
    assert fh.HashGridDesc.per_level_scale.offset == 20 and fh.HashGridDesc.x_stride.offset == 32 and fh.HashGridDesc.dx_stride.offset == 56
    assert th.LDS_BYTES == int(re.search(r"#define GSR_HASHGRID_LDS_BYTES \((\d+) \* 1024\)", open(HDR).read()).group(1)) * 1024


def test_entry_points_refuse_before_any_device_work():
    L = _lib()
    p = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused or has nothing to do
    big = ctypes.c_size_t(1 << 30)

    def fwd(word, d=None, x=p, table=p, y=p):
        d = _desc() if d is None else d
        assert L.gsr_hashgrid_forward(ctypes.byref(d) if d is not False else None, x, table, y, None) == -1, word
        text = L.gsr_last_error().decode()
        assert text.startswith("gsr_hashgrid_forward:") and word in text, text

    def bwd(word, d=None, x=p, table=p, dy=p, dx=p, dtable=p, scratch=p, nbytes=big):
        d = _desc() if d is None else d
        assert L.gsr_hashgrid_backward(ctypes.byref(d), x, table, dy, dx, dtable, scratch, nbytes, None) == -1, word
        text = L.gsr_last_error().decode()
        assert text.startswith("gsr_hashgrid_backward:") and word in text, text

    fwd("desc is NULL", d=False)
    fwd("negative count", _desc(N=-1))
    for D in (1, 5):
        fwd("D must be 2, 3 or 4", _desc((D, 3, 2, 12, 8, 2.0)))
    for Lv in (0, 33):
        fwd("L must lie in 1..32", _desc((3, Lv, 2, 12, 8, 2.0)))
    for F in (0, 3, 16):
        fwd("F must be 1, 2, 4 or 8", _desc((3, 3, F, 12, 8, 2.0)))
    fwd("base_resolution must be at least 1", _desc((3, 3, 2, 12, 0, 2.0)))
    for s in (0.5, float("nan"), float("inf")):
        fwd("per_level_scale must be", _desc((3, 3, 2, 12, 8, s)))
    for T in (0, 25):
        fwd("log2_hashmap_size must lie in 1..24", _desc((3, 3, 2, T, 8, 2.0)))
    fwd("finest resolution exceeds 2^30", _desc((3, 32, 2, 12, 16, 2.0)))
    fwd("stride is smaller", _desc(xs=2))
    fwd("stride is smaller", _desc(ys=5))
    for kw in (dict(x=None), dict(table=None), dict(y=None)):
        fwd("is NULL", **kw)
    bwd("negative count", _desc(N=-1))
    bwd("stride is smaller", _desc(dys=5))
    bwd("stride is smaller", _desc(dxs=2))
    bwd("is NULL", dy=None)
    bwd("scratch is NULL", scratch=None)
    bwd("16-byte aligned", scratch=ctypes.c_void_p(4104))
    lo, full = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.gsr_hashgrid_scratch_bytes(ctypes.byref(_desc()), ctypes.byref(lo), ctypes.byref(full)) == 0
    bwd("below the minimum", nbytes=ctypes.c_size_t(lo.value - 1))
    d0 = _desc(N=0)
    assert L.gsr_hashgrid_forward(ctypes.byref(d0), None, None, None, None) == 0   # nothing to do, whatever the pointers
    assert L.gsr_hashgrid_backward(ctypes.byref(d0), None, None, None, None, None, None, 0, None) == 0
    assert L.gsr_hashgrid_backward(ctypes.byref(_desc()), p, p, p, None, None, None, 0, None) == 0   # nothing wanted: nothing done


def test_scratch_sizes():
    L = _lib()
    lo, full = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert L.gsr_hashgrid_scratch_bytes(ctypes.byref(_desc((3, 3, 3, 12, 8, 2.0))), ctypes.byref(lo), ctypes.byref(full)) == -1
    assert lo.value == 0 and full.value == 0
    for name, cfg in th.CONFIGS.items():
        lay = th.layout(cfg)
        assert L.gsr_hashgrid_scratch_bytes(ctypes.byref(_desc(cfg, N=5)), ctypes.byref(lo), ctypes.byref(full)) == 0
        assert lo.value == 256 + max(lay["sizes"]) * cfg[2] * 8 and full.value == 256 + lay["total"] * cfg[2] * 8, name
        a = ctypes.c_size_t()
        assert L.gsr_hashgrid_scratch_bytes(ctypes.byref(_desc(cfg, N=5000000)), ctypes.byref(a), None) == 0 and a.value == lo.value   # not of size N
    assert L.gsr_hashgrid_scratch_bytes(ctypes.byref(_desc(DEFAULT)), ctypes.byref(lo), ctypes.byref(full)) == 0
    assert lo.value == 256 + (8 << 20) and full.value < 256 << 20


CONFIG_ITEMS = sorted(th.CONFIGS.items()) + [("default", DEFAULT), ("finest4096", (3, 16, 2, 19, 16, 1.4472692012786865)),
                                             ("d4", (4, 16, 2, 19, 8, 1.38)), ("d2", (2, 16, 4, 19, 16, 1.51)), ("one", (2, 1, 1, 1, 1, 1.0))]


@pytest.mark.parametrize("name,cfg", CONFIG_ITEMS)
def test_layout_equals_the_librarys(name, cfg):
    import fused_hashgrid as fh
    D, L, F, T, base, pls = cfg
    lay = th.layout(cfg)
    off, res, hashed, total = fh.level_layout(D, L, F, T, base, pls)
    assert off == lay["offs"] and res == lay["res"] and hashed == lay["hashed"] and total == lay["total"]
    assert fh.level_paths(D, L, F, T, base, pls) == [fh.PATH_LDS if v else fh.PATH_DIRECT for v in lay["lds"]]
    d = fh.check_config(D, L, F, T, base, pls)
    scales = np.array([fh._lib().gsr_hashgrid_level_scale(ctypes.byref(d), l) for l in range(L)], np.float32)
    assert np.array_equal(scales, lay["scales"])
    assert fh._entries(d) == total
    assert fh._lib().gsr_hashgrid_level_path(ctypes.byref(d), L) == -1 and fh._lib().gsr_hashgrid_level_path(ctypes.byref(d), -1) == -1
    assert all(s % 8 == 0 or s == 1 << T for s in lay["sizes"]) and all(b >= a for a, b in zip(lay["res"], lay["res"][1:]))


def test_the_fixtures_cover_what_they_promise():
    lay = th.layout(th.CONFIGS["all3"])
    assert lay["res"] == [2, 4, 8, 16, 32] and lay["sizes"] == [8, 64, 512, 4096, 4096]
    assert lay["hashed"] == [False, False, False, False, True]      # res 16: 16^3 == 2^12 exactly, still dense; the next level hashed
    assert lay["lds"] == [True, True, True, False, False]            # a dense level on each side of the LDS budget
    assert 512 * 8 * 8 <= th.LDS_BYTES < 4096 * 8 * 8
    lay = th.layout(th.CONFIGS["seam3"])
    assert lay["res"][1] ** 3 == lay["sizes"][1] == 1 << 12 and lay["hashed"] == [False, False, True] and lay["lds"] == [True, True, False]
    lay = th.layout(th.CONFIGS["budget2"])
    assert lay["hashed"] == [False, False, True] and lay["lds"] == [True, False, False]
    assert lay["sizes"][0] * 2 * 8 <= th.LDS_BYTES < lay["sizes"][1] * 2 * 8
    lay = th.layout(th.CONFIGS["tiny2"])
    assert lay["sizes"] == [8, 16, 16] and lay["hashed"] == [False, False, True]   # 16-entry levels, one dense and one hashed
    kinds = {(cfg[0], "dense" if not any(h) else "hashed" if all(h) else "seam") for cfg in th.CONFIGS.values() for h in [th.layout(cfg)["hashed"]]}
    assert kinds == {(D, k) for D in (2, 3, 4) for k in ("dense", "seam", "hashed")}
    assert {c[2] for c in th.CONFIGS.values()} == {1, 2, 4, 8} and {c[1] for c in th.CONFIGS.values()} >= {1, 3, 8}
    assert {c[3] for c in th.CONFIGS.values()} >= {4, 10, 12}
    assert any(s & (s - 1) for c in th.CONFIGS.values() for s in th.layout(c)["sizes"])   # a size that is no power of two: the real mod


# ---- the references --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all3", "budget2", "hashed4", "dense2", "tiny2"])
def test_float64_rule_equals_autograd_of_the_torch_version(name):
    c = th.general_fixture(name, N=200)
    ref = th.ref64(c["x"], c["table"], c["dy"], c["cfg"])
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    table = torch.from_numpy(c["table"]).double().requires_grad_(True)
    y = th.hash_grid_torch(x, table, c["cfg"])
    (y * torch.from_numpy(c["dy"]).double()).sum().backward()
    close = lambda a, b: np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    assert close(y.detach().numpy(), ref["y"])
    assert close(table.grad.numpy(), ref["dtable"])
    void = ~np.isfinite(c["x"]).all(1)
    gx = x.grad.numpy()
    assert void.sum() == 3 and (gx[void] == 0).all()
    assert close(gx[~void], ref["dx"][~void])
    assert (ref["dx"][void] == 0).all() and (ref["y"][void] == 0).all()
    outside = (c["x"] < 0) | (c["x"] > 1)
    assert outside.sum() >= 3 and (ref["dx"][outside] == 0).all()


def _round_f32(fr):
    """A Fraction -> the nearest float32 (ties to even), as a Fraction; exact arithmetic throughout (normal range only)"""
    if fr == 0:
        return Fraction(0)
    s, a = (-1 if fr < 0 else 1), abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and -126 <= e <= 127
    ulp = Fraction(2) ** (e - 23)
    return s * round(a / ulp) * ulp   # round(Fraction) rounds ties to even


@pytest.mark.parametrize("name,spread", [("tiny2", False), ("seam3", False), ("hashed4", True)])
def test_integer_emulation_equals_exact_rationals(name, spread):
    c = th.general_fixture(name, N=40, outside=True)
    cfg, x, dy = c["cfg"], c["x"], c["dy"].copy()
    if spread:
        dy *= np.exp2(np.random.default_rng(5).integers(-30, 31, dy.shape)).astype(np.float32)
    D, L, F = cfg[:3]
    lay = th.layout(cfg)
    got, q, n_e = th.emulate_dtable(x, dy, cfg, info=True)
    S = [[Fraction(0)] * F for _ in range(lay["total"])]
    exact = [[Fraction(0)] * F for _ in range(lay["total"])]
    count = np.zeros(lay["total"], np.int64)
    for l in range(L):
        void, idx, w, _, _ = th.level_terms(x, lay, l)
        for i in range(len(x)):
            if void[i]:
                continue
            for k in range(1 << D):
                e = lay["offs"][l] + int(idx[i, k])
                count[e] += 1
                for f in range(F):
                    term = Fraction(float(w[i, k])) * Fraction(float(dy[i, l * F + f]))
                    exact[e][f] += term
                    S[e][f] += round(term * Fraction(2) ** q)
    assert np.array_equal(count, n_e)
    for e in range(lay["total"]):
        for f in range(F):
            assert abs(S[e][f]) <= 2 ** 62
            want = _round_f32(S[e][f] / Fraction(2) ** q)
            assert Fraction(float(got[e, f])) == want, (e, f)
            # the header's bound against the exact sum: n_e 2^-(q+1), then one float32 rounding
            assert abs(S[e][f] / Fraction(2) ** q - exact[e][f]) <= int(n_e[e]) * Fraction(2) ** (-(q + 1))


def test_integer_emulation_special_cases():
    c = th.general_fixture("seam3", N=50)
    total, F = th.layout(c["cfg"])["total"], c["cfg"][2]
    z = th.emulate_dtable(c["x"], np.zeros_like(c["dy"]), c["cfg"])
    assert z.shape == (total, F) and not z.any() and not np.signbit(z).any()
    for bad in (np.inf, -np.inf, np.nan):
        dy = c["dy"].copy()
        dy[17, 2] = bad
        assert np.isnan(th.emulate_dtable(c["x"], dy, c["cfg"])).all()
    assert th.quantum(np.array([[0.75, -3.0]], np.float32), 1000, 3) == ("sum", 62 - 13 - 2)
    assert th.quantum(np.array([[2.0 ** -149]], np.float32), 1, 2) == ("sum", 62 - 2 + 148)


@pytest.mark.parametrize("name", th.INTEGER_CONFIGS)
def test_integer_fixtures_are_exact(name):
    c = th.integer_fixture(name)
    cfg, x = c["cfg"], c["x"]
    lay = th.layout(cfg)
    weights = set()
    for l in range(lay["L"]):
        weights |= set(np.unique(th.level_terms(x, lay, l)[3]).tolist())
    # growth 1 at base 5 (dense3): x scale_l + 0.5 is an integer and a half throughout
    assert weights == ({0.5} if name == "dense3" else {0.0, 0.25, 0.5, 0.75, 1.0})
    assert (x == 0).all(1).any() and (x == 1).all(1).any()   # the first cell, and the top cell with its +1 corners
    y, und = th.emulate_y(x, c["table"], cfg)
    ref = th.ref64(x, c["table"], c["dy"], cfg)
    assert not und.any() and np.array_equal(y.astype(np.float64), ref["y"])                      # y: exact in float32
    assert np.array_equal(th.emulate_dtable(x, c["dy"], cfg).astype(np.float64), ref["dtable"])   # dtable: exact in int64 and float32
    assert np.abs(ref["dx"]).max() > 0 and np.array_equal(ref["dx"] * 4 ** lay["D"], np.rint(ref["dx"] * 4 ** lay["D"]))   # dx: an exact double sum


@pytest.mark.parametrize("name", sorted(th.CONFIGS))
def test_general_fixtures_are_decided_and_robust(name):
    c = th.general_fixture(name)
    fragile = th.fragile_rows(c["x"], c["cfg"])
    assert fragile.mean() <= 0.02, fragile.mean()
    y, und = th.emulate_y(c["x"], c["table"], c["cfg"])
    assert und.mean() <= 0.001
    ref = th.ref64(c["x"], c["table"], None, c["cfg"])
    assert np.abs(y - ref["y"]).max() <= 2.0 ** -19 * np.abs(c["table"]).max()   # the chain is the rule, to float32 accuracy


# ---- the Python surface refuses before any kernel or library call ------------------------------------------------------------------
def test_python_refusals_without_a_device():
    import fused_hashgrid as fh
    total = th.layout(DEFAULT)["total"]
    x = torch.zeros((10, 3))
    table = torch.zeros((total, 2))
    for kw, exc, word in [(dict(levels=0), ValueError, "levels must lie in 1..32"), (dict(levels=33), ValueError, "levels"),
                          (dict(levels=2.0), TypeError, "levels must be an int"), (dict(features=3), ValueError, "features must be 1, 2, 4 or 8"),
                          (dict(features=True), TypeError, "features must be an int"), (dict(log2_hashmap_size=0), ValueError, "log2_hashmap_size"),
                          (dict(log2_hashmap_size=25), ValueError, "log2_hashmap_size"), (dict(base_resolution=0), ValueError, "base_resolution"),
                          (dict(per_level_scale=0.9), ValueError, "per_level_scale"), (dict(per_level_scale=float("nan")), ValueError, "per_level_scale"),
                          (dict(per_level_scale="2"), TypeError, "per_level_scale must be a float"),
                          (dict(levels=32), ValueError, "finest resolution")]:
        with pytest.raises(exc, match=word):
            fh.hash_grid(x, table, **kw)
        with pytest.raises(exc, match=word):
            fh.hash_grid_and_grads(x, table, **kw)
    with pytest.raises(TypeError, match="x must be a tensor"):
        fh.hash_grid(x.numpy(), table)
    with pytest.raises(TypeError, match="table must be a tensor"):
        fh.hash_grid(x, None)
    with pytest.raises(RuntimeError, match="x must have two dimensions"):
        fh.hash_grid(x[0], table)
    with pytest.raises(RuntimeError, match="x must be float32"):
        fh.hash_grid(x.double(), table)
    with pytest.raises(RuntimeError, match="table must be float32"):
        fh.hash_grid(x, table.half())
    for D in (1, 5):
        with pytest.raises(ValueError, match="x must have 2, 3 or 4 columns"):
            fh.hash_grid(torch.zeros((10, D)), table)
    with pytest.raises(RuntimeError, match="table must have 2 columns"):
        fh.hash_grid(x, torch.zeros((total, 4)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fh.hash_grid(x, table)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fh.hash_grid_and_grads(x, table, torch.zeros((10, 32)))
    with pytest.raises(RuntimeError, match=f"table must have {total} rows"):
        fh.hash_grid(x, torch.zeros((total - 8, 2)))
    for kw, exc, word in [(dict(in_dim=1), ValueError, "in_dim must lie in 2..4"), (dict(in_dim=5), ValueError, "in_dim"),
                          (dict(in_dim=3, finest_resolution=512, per_level_scale=1.5), ValueError, "not both"),
                          (dict(in_dim=3, finest_resolution=8), ValueError, "finest_resolution"), (dict(in_dim=3, features=5), ValueError, "features")]:
        with pytest.raises(exc, match=word):
            fh.HashGrid(**kw)
    for kw in (dict(in_dim=7), dict(in_dim=3, levels=33), dict(in_dim=3, features=3), dict(in_dim=3, per_level_scale=0.5)):
        with pytest.raises(ValueError):
            fh.level_layout(**kw)


def test_module_without_a_device():
    import fused_hashgrid as fh
    g = fh.HashGrid(3, levels=8, features=2, log2_hashmap_size=12, base_resolution=4, finest_resolution=128)
    lay = th.layout((3, 8, 2, 12, 4, g.per_level_scale))
    assert g.out_dim == 16 and tuple(g.table.shape) == (lay["total"], 2) and g.table.dtype == torch.float32
    assert [p is g.table for p in g.parameters()] == [True]
    assert float(g.table.detach().abs().max()) <= 1e-4 and float(g.table.detach().std()) > 3e-5
    assert abs(g.per_level_scale - 32 ** (1 / 7)) < 1e-6 and lay["res"][0] == 4 and lay["res"][-1] in (128, 129)
    assert fh.HashGrid(2).per_level_scale == 2.0 and fh.HashGrid(2, levels=1, finest_resolution=16).per_level_scale == 1.0
    assert "entries=" in repr(g)


# ---- the kernels' resource usage ---------------------------------------------------------------------------------------------------
def test_every_kernel_compiles_without_scratch():
    """One device-only compile of hashgrid.hip with the Makefile's flags: every kernel, every instantiation, 0 bytes of scratch"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^hashgrid\.o: hashgrid\.hip \$\(HDRS\)\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\)", mk, flags=re.M), "hashgrid.o must be built with $(EXACT)"
    assert mk.count("vq mlp hashgrid),$(EXACT)") == 2, "make variant and make audit must compile hashgrid uncontracted"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "hashgrid.hip", "-o", os.devnull], cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == 50, names   # max, convert, and 12 (D, F) instantiations each of forward, dx, direct and LDS
    for kind in ("forward_kernel", "dx_kernel", "grad_direct_kernel", "grad_lds_kernel"):
        assert sum(kind in n for n in names) == 12, kind
    assert all(v == 0 for v in scratch), dict(zip(names, scratch))
