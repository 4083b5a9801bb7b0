"""CPU: the references of the plane-grid encoding against each other, against F.grid_sample and against exact rationals, the fixtures'
promises, the layout against the library's host code, the C ABI's refusals, every Python refusal, and hexplane.hip's resource usage.
No GPU is touched."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import torch_hexplane as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsr_hexplane.h")
CSRC = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "csrc")
LIB = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "libgsr_hip.so")
NAMES = ["gsr_hexplane_backward", "gsr_hexplane_forward", "gsr_hexplane_layout", "gsr_hexplane_level_path", "gsr_hexplane_regularizer",
         "gsr_hexplane_scratch_bytes"]
ALL = {**th.CONFIGS, **th.INTEGER_CONFIGS}


def _lib():
    if not os.path.exists(LIB):
        __graft_entry__.build()
    import fused_hexplane
    return fused_hexplane._lib()


def _cfg(c):
    import fused_hexplane as fh
    return fh.HexPlaneConfig(c.D, c.C, c.res, c.concat)


def _desc(c=th.CONFIGS["odd_d4"], N=10, xs=None, ys=None, dys=None, dxs=None, **over):
    """A desc built field by field, so that values a HexPlaneConfig refuses reach the library"""
    import fused_hexplane as fh
    d = fh.HexPlaneDesc(N=N, D=c.D, L=len(c.res), C=c.C, concat=int(c.concat))
    for l, level in enumerate(c.res):
        for a, r in enumerate(level):
            d.res[l][a] = r
    for k, v in over.items():
        setattr(d, k, v)
    cols = th.out_dim(c)
    d.x_stride = c.D if xs is None else xs
    d.y_stride = cols if ys is None else ys
    d.dy_stride = cols if dys is None else dys
    d.dx_stride = c.D if dxs is None else dxs
    return d


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_is_c99(tmp_path):
    src = tmp_path / "use_hexplane.c"
    src.write_text('#include "gsr_hexplane.h"\n#include "gsr_hexplane.h"\n'
                   "int use(void) { gsr_hexplane_desc d; d.N = 0; return (int)(sizeof(&gsr_hexplane_forward) + sizeof(&gsr_hexplane_backward) + sizeof d) + "
                   "GSR_HEXPLANE_MAX_LEVELS + GSR_HEXPLANE_PATH_LDS + GSR_HEXPLANE_LDS_BYTES + GSR_HEXPLANE_REG_SCRATCH_BYTES + d.N; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "use_hexplane.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_library_exports_the_names_of_the_header():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr))) == NAMES
    L = _lib()
    for n in NAMES:
        assert hasattr(L, n), n


def test_the_record_and_the_constants_are_the_headers():
    import fused_hexplane as fh
    assert ctypes.sizeof(fh.HexPlaneDesc) == 4 * 5 + 4 * 32 + 4 + 8 * 4   # five ints, res[8][4], padding, four strides
    assert fh.HexPlaneDesc.res.offset == 20 and fh.HexPlaneDesc.x_stride.offset == 152 and fh.HexPlaneDesc.dx_stride.offset == 176
    hdr = open(HDR).read()
    value = lambda name: eval(re.search(r"#define " + name + r" (.+)", hdr).group(1))
    assert value("GSR_HEXPLANE_LDS_BYTES") == th.LDS_BYTES == fh.LDS_BYTES
    assert value("GSR_HEXPLANE_MAX_LEVELS") == fh.MAX_LEVELS and value("GSR_HEXPLANE_MAX_RES") == fh.MAX_RES
    assert value("GSR_HEXPLANE_REG_SCRATCH_BYTES") == fh.REG_SCRATCH
    assert (value("GSR_HEXPLANE_PATH_DIRECT"), value("GSR_HEXPLANE_PATH_LDS")) == (fh.PATH_DIRECT, fh.PATH_LDS)


def test_entry_points_refuse_before_any_device_work():
    L = _lib()
    p = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused or has nothing to do
    big = ctypes.c_size_t(1 << 30)
    c = th.CONFIGS["odd_d4"]

    def fwd(word, d=None, x=p, table=p, y=p):
        d = _desc() if d is None else d
        assert L.gsr_hexplane_forward(ctypes.byref(d) if d is not False else None, x, table, y, None) == -1, word
        text = L.gsr_last_error().decode()
        assert text.startswith("gsr_hexplane_forward:") and word in text, text

    def bwd(word, d=None, x=p, table=p, dy=p, dx=p, dtable=p, scratch=p, nbytes=big):
        d = _desc() if d is None else d
        assert L.gsr_hexplane_backward(ctypes.byref(d), x, table, dy, dx, dtable, scratch, nbytes, None) == -1, word
        text = L.gsr_last_error().decode()
        assert text.startswith("gsr_hexplane_backward:") and word in text, text

    def reg(word, d=None, table=p, value=p, scratch=p, nbytes=ctypes.c_size_t(65536)):
        d = _desc() if d is None else d
        assert L.gsr_hexplane_regularizer(ctypes.byref(d) if d is not False else None, table, 1.0, 1.0, 1.0, 1.0, 1.0, value, None, scratch, nbytes, None) == -1, word
        text = L.gsr_last_error().decode()
        assert text.startswith("gsr_hexplane_regularizer:") and word in text, text

    fwd("desc is NULL", d=False)
    fwd("negative count", _desc(N=-1))
    for D in (2, 5):
        fwd("D must be 3 or 4", _desc(D=D))
    for Lv in (0, 9):
        fwd("L must lie in 1..8", _desc(L=Lv))
    for C in (0, 2, 6, 68):
        fwd("C must be a multiple of 4 in 4..64", _desc(C=C))
    for r in (1, 4097, -3):
        d = _desc()
        d.res[0][2] = r
        fwd("a resolution must lie in 2..4096", d)
    d = _desc(c._replace(D=3, res=((3, 5, 4),)))
    d.res[0][3] = 0                           # beyond D: not read
    assert L.gsr_hexplane_scratch_bytes(ctypes.byref(d), None, None) == 0
    fwd("stride is smaller", _desc(xs=3))
    fwd("stride is smaller", _desc(ys=11))
    fwd("stride is smaller", _desc(c._replace(res=c.res * 2), ys=23))   # concat: L C columns
    assert L.gsr_hexplane_forward(ctypes.byref(_desc(c._replace(res=c.res * 2, concat=False), N=0, ys=12)), None, None, None, None) == 0   # summed: C columns
    for kw in (dict(x=None), dict(table=None), dict(y=None)):
        fwd("is NULL", **kw)
    bwd("negative count", _desc(N=-1))
    bwd("stride is smaller", _desc(dys=11))
    bwd("stride is smaller", _desc(dxs=3))
    bwd("is NULL", dy=None)
    bwd("scratch is NULL", scratch=None)
    bwd("16-byte aligned", scratch=ctypes.c_void_p(4104))
    lo, full = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.gsr_hexplane_scratch_bytes(ctypes.byref(_desc()), ctypes.byref(lo), ctypes.byref(full)) == 0
    bwd("below the minimum", nbytes=ctypes.c_size_t(lo.value - 1))
    d0 = _desc(N=0)
    assert L.gsr_hexplane_forward(ctypes.byref(d0), None, None, None, None) == 0   # nothing to do, whatever the pointers
    assert L.gsr_hexplane_backward(ctypes.byref(d0), None, None, None, None, None, None, 0, None) == 0
    assert L.gsr_hexplane_backward(ctypes.byref(_desc()), p, p, p, None, None, None, 0, None) == 0   # nothing wanted: nothing done
    reg("desc is NULL", d=False)
    reg("C must be", _desc(C=5))
    reg("is NULL", table=None)
    reg("is NULL", value=None)
    reg("scratch is NULL", scratch=None)
    reg("16-byte aligned", scratch=ctypes.c_void_p(4104))
    reg("below the minimum", nbytes=ctypes.c_size_t(65535))
    assert L.gsr_hexplane_layout(ctypes.byref(_desc()), None) == -1 and L.gsr_last_error().decode().startswith("gsr_hexplane_layout:")
    assert L.gsr_hexplane_layout(ctypes.byref(_desc(D=7)), None) == -1


@pytest.mark.parametrize("name", sorted(ALL))
def test_layout_paths_and_scratch_equal_the_librarys(name):
    import fused_hexplane as fh
    c = ALL[name]
    cfg = _cfg(c)
    off, shp, tot = fh.plane_layout(cfg)
    assert off == th.offsets(c) and tot == th.total(c) == cfg.total() and shp == [(rb, ra) for *_, rb, ra in th.shapes(c)]
    assert cfg.planes == tuple(th.planes(c)) and cfg.out_dim == th.out_dim(c)
    assert fh.level_paths(cfg) == [[fh.PATH_LDS if v else fh.PATH_DIRECT for v in level] for level in th.lds(c)]
    L = _lib()
    d = cfg.desc(5)
    assert L.gsr_hexplane_level_path(ctypes.byref(d), len(c.res), 0) == -1 and L.gsr_hexplane_level_path(ctypes.byref(d), 0, len(cfg.planes)) == -1
    assert L.gsr_hexplane_level_path(ctypes.byref(d), -1, 0) == -1 and L.gsr_hexplane_level_path(ctypes.byref(d), 0, -1) == -1
    lo, full = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert L.gsr_hexplane_scratch_bytes(ctypes.byref(d), ctypes.byref(lo), ctypes.byref(full)) == 0
    sizes = np.diff(off)
    assert lo.value == 512 + int(sizes.max()) * 8 and full.value == 512 + tot * 8
    a = ctypes.c_size_t()
    assert L.gsr_hexplane_scratch_bytes(ctypes.byref(cfg.desc(5000000)), ctypes.byref(a), None) == 0 and a.value == lo.value   # not of size N
    assert L.gsr_hexplane_scratch_bytes(ctypes.byref(_desc(C=5)), ctypes.byref(lo), ctypes.byref(full)) == -1 and lo.value == 0 and full.value == 0


def test_pack_and_unpack_round_trip_and_mean_what_grid_sample_means():
    import fused_hexplane as fh
    c = th.CONFIGS["odd_d4"]
    cfg = _cfg(c)
    table = torch.arange(th.total(c), dtype=torch.float32)
    grids = fh.unpack_planes(table, cfg)
    assert [tuple(g.shape) for g in grids[0]] == [(1, 12, rb, ra) for *_, rb, ra in th.shapes(c)]
    assert [tuple(g.shape) for g in grids[0]] == [(1, 12, 5, 3), (1, 12, 4, 3), (1, 12, 2, 3), (1, 12, 4, 5), (1, 12, 2, 5), (1, 12, 2, 4)]
    assert torch.equal(fh.pack_planes(grids), table)
    assert all(torch.equal(a, b) for a, b in zip(grids[0], th.unpack(table, c)[0]))
    off = th.offsets(c)
    k, ib, ia, ch = 3, 2, 4, 7                       # plane (1, 2): res_a = 5 (axis 1), res_b = 4 (axis 2)
    assert float(grids[0][k][0, ch, ib, ia]) == float(table[off[k] + (ib * 5 + ia) * 12 + ch])
    copies = [[g.clone() for g in level] for level in grids]
    assert torch.equal(fh.pack_planes(copies), table)
    with pytest.raises(RuntimeError, match="one flat tensor"):
        fh.unpack_planes(table[:-1], cfg)
    assert fh.resolutions((64, 64, 64, 25), (1, 2)) == ((64, 64, 64, 25), (128, 128, 128, 25))
    assert fh.resolutions((8, 9, 10), (1, 3)) == ((8, 9, 10), (24, 27, 30))


def test_the_fixtures_cover_what_they_promise():
    assert th.lds(th.CONFIGS["seam_d4"]) == [[True] * 6, [False] + [True] * 5]
    assert 64 * 64 * 4 * 8 == th.LDS_BYTES < 65 * 64 * 4 * 8
    assert th.lds(th.CONFIGS["direct_d3"])[0] == [False, True, True] and th.lds(th.CONFIGS["direct_d4"])[0][0] is False
    assert th.lds(th.INTEGER_CONFIGS["int_seam"]) == [[False, True, True]]
    assert {c.D for c in th.CONFIGS.values()} == {3, 4} and {c.C for c in th.CONFIGS.values()} == {4, 12, 32, 64}
    assert {len(c.res) for c in th.CONFIGS.values()} == {1, 2, 3} and {c.concat for c in th.CONFIGS.values()} == {True, False}
    assert th.CONFIGS["odd_d4"].res == ((3, 5, 4, 2),) and th.CONFIGS["r2_d4"].res == ((2, 2, 2, 2),)
    assert th.CONFIGS["multi_d4"].res == ((8, 8, 8, 4), (16, 16, 16, 4))
    c = th.one_cell_fixture("seam_d4")
    for l in range(2):
        i0, _ = th.level_terms(c["x"], c["cfg"], l)
        assert (i0 == i0[0]).all() if l == 0 else True
    g = th.general_fixture("odd_d4")
    assert (g["x"] == -1).any() and (g["x"] == 1).any() and (g["x"] > 1).any() and (g["x"] < -1).any() and (~np.isfinite(g["x"])).any(1).sum() == 3


# ---- the references --------------------------------------------------------------------------------------------------------------------
def _autograd64(c):
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    table = torch.from_numpy(c["table"]).double().requires_grad_(True)
    y = th.hex_plane_torch(x, table, c["cfg"])
    (y * torch.from_numpy(c["dy"]).double()).sum().backward()
    return y.detach().numpy(), x.grad.numpy(), table.grad.numpy()


@pytest.mark.parametrize("name", ["r2_d4", "odd_d4", "multi_d4", "multi_d3", "direct_d3"])
def test_float64_rule_equals_autograd_of_grid_sample(name):
    """The rule with frac left in double is F.grid_sample in float64, to 1e-12: y, dx (u exactly -1 and +1 and beyond included: the
    clamped axes' zeros are torch's), dtable.  With the rule's float32 frac it lies within the float32 rounding of the weights."""
    c = th.general_fixture(name, N=200)
    y, gx, gt = _autograd64(c)
    ref = th.ref64(c["x"], c["table"], c["dy"], c["cfg"], frac32=False)
    close = lambda a, b, tol=1e-12: np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())
    assert close(ref["y"], y) and close(ref["dtable"], gt) and close(ref["dx"], gx)
    void, clamped = th.rows(c["x"])
    assert void.sum() == 3 and (gx[void] == 0).all() and (ref["dx"][void] == 0).all() and (ref["y"][void] == 0).all()
    edge = clamped & ~void[:, None]
    assert edge.sum() >= 6 and (gx[edge] == 0).all() and (ref["dx"][edge] == 0).all()
    assert np.abs(gx[~void][:, 0]).max() > 0 and np.abs(gx[:, c["cfg"].D - 1]).max() > 0   # every column has a gradient, the last included
    r32 = th.ref64(c["x"], c["table"], c["dy"], c["cfg"], frac32=True)
    assert close(r32["y"], y, 1e-5) and close(r32["dx"], gx, 1e-4) and close(r32["dtable"], gt, 1e-5)


@pytest.mark.parametrize("name", sorted(th.INTEGER_CONFIGS))
def test_integer_fixtures_are_exact_and_equal_grid_sample(name):
    """frac is exact in float32 here, so the rule as the kernels run it equals grid_sample's float64 too"""
    c = th.integer_fixture(name)
    cfg, x = c["cfg"], c["x"]
    fr = set()
    for l in range(len(cfg.res)):
        fr |= set(np.unique(th.level_terms(x, cfg, l)[1]).tolist())
    assert fr == {0.0, 0.5, 1.0}                          # nodes and half nodes; 1 at u = +1 alone, where i0 = res - 2
    assert (x == -1).all(1).any() and (x == 1).all(1).any()
    ref = th.ref64(x, c["table"], c["dy"], cfg)
    y64, gx, gt = _autograd64(c)
    assert np.array_equal(ref["y"], y64) and np.array_equal(ref["dtable"], gt) and np.array_equal(ref["dx"], gx)
    y, und, _ = th.emulate_y(x, c["table"], cfg)
    assert not und.any() and np.array_equal(y.astype(np.float64), ref["y"])                                  # y: exact in float32
    assert np.array_equal(th.emulate_dtable(x, c["table"], c["dy"], cfg).astype(np.float64), ref["dtable"])   # dtable: exact in int64 and float32
    assert np.abs(ref["dx"]).max() > 0 and np.array_equal(ref["dx"].astype(np.float32).astype(np.float64), ref["dx"])
    assert np.abs(ref["y"]).max() < 2 ** 24 and np.abs(ref["dtable"]).max() < 2 ** 24


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


@pytest.mark.parametrize("name,spread", [("r2_d4", False), ("odd_d4", True), ("direct_d3", True)])
def test_integer_emulation_equals_exact_rationals(name, spread):
    c = th.general_fixture(name, N=40)
    cfg, x, table, dy = c["cfg"], c["x"], c["table"], c["dy"].copy()
    if name == "direct_d3":   # the big plane would take minutes in rationals: a small one of the same kind
        cfg = cfg._replace(res=((7, 6, 2), (3, 5, 4)))
        table = table[:th.total(cfg)]
    if spread:
        dy *= np.exp2(np.random.default_rng(5).integers(-30, 31, dy.shape)).astype(np.float32)
    C, P = cfg.C, len(th.planes(cfg))
    off = th.offsets(cfg)
    got, q, n_e, worst = th.emulate_dtable(x, table, dy, cfg, info=True)
    assert 0 < worst <= 1
    _, _, ps = th.emulate_y(x, table, cfg)
    void, _ = th.rows(x)
    S, exact, mod = [0] * off[-1], [Fraction(0)] * off[-1], [Fraction(0)] * off[-1]
    count = np.zeros(off[-1] // C, np.int64)
    for l in range(len(cfg.res)):
        i0, frac = th.level_terms(x, cfg, l)
        for k, (a, b) in enumerate(th.planes(cfg)):
            j = l * P + k
            nodes, w = th.corner_nodes(i0, a, b, cfg.res[l][a]), th.weights32(frac, a, b)
            for i in np.flatnonzero(~void):
                for n in range(4):
                    count[off[j] // C + nodes[i, n]] += 1
                    for ch in range(C):
                        g, gx = float(th.level_dy(dy, cfg, l)[i, ch]), Fraction(float(th.level_dy(dy, cfg, l)[i, ch]))
                        for jj in range(P):
                            if jj != k:
                                g, gx = g * float(ps[l][jj][i, ch]), gx * Fraction(float(ps[l][jj][i, ch]))
                        e = off[j] + int(nodes[i, n]) * C + ch
                        S[e] += round(Fraction(float(w[i, n]) * g) * Fraction(2) ** q[l][k])   # the double product, scaled exactly, to nearest even
                        exact[e] += Fraction(float(w[i, n])) * gx
                        mod[e] += abs(Fraction(float(w[i, n])) * gx)
    assert np.array_equal(count, n_e)
    for j in range(len(off) - 1):
        qq = q[j // P][j % P]
        for e in range(off[j], off[j + 1]):
            assert abs(S[e]) <= 2 ** 62
            assert Fraction(float(got[e])) == _round_f32(Fraction(S[e]) / Fraction(2) ** qq), e
            # the header's bound against the exact sum: n_e 2^-(q+1), the double roundings of the products, then one float32 rounding
            assert abs(Fraction(S[e]) / Fraction(2) ** qq - exact[e]) <= int(n_e[e // C]) * Fraction(2) ** (-(qq + 1)) + 7 * Fraction(2) ** -53 * mod[e]


@pytest.mark.parametrize("name", sorted(th.CONFIGS))
def test_the_scale_holds_every_term_and_the_fixtures_are_decided(name):
    """|t| <= 2^(62 - B) on every fixture (the scale needs no forward pass and must still hold), at most 0.1 % undecided elements of y,
    and the float32 chain is the rule to float32 accuracy"""
    for c in (th.general_fixture(name), th.one_cell_fixture(name)):
        y, und, _ = th.emulate_y(c["x"], c["table"], c["cfg"])
        assert und.mean() <= 0.001, und.mean()
        _, q, _, worst = th.emulate_dtable(c["x"], c["table"], c["dy"], c["cfg"], info=True)
        assert 0 < worst <= 1, worst
        ref = th.ref64(c["x"], c["table"], None, c["cfg"])
        P = len(th.planes(c["cfg"]))
        assert np.abs(y - ref["y"]).max() <= 2.0 ** -19 * np.abs(c["table"]).max() ** P * len(c["cfg"].res)


def test_integer_emulation_special_cases():
    c = th.general_fixture("odd_d4", N=50)
    cfg = c["cfg"]
    z = th.emulate_dtable(c["x"], c["table"], np.zeros_like(c["dy"]), cfg)
    assert z.shape == (th.total(cfg),) and not z.any() and not np.signbit(z).any()
    for bad in (np.inf, -np.inf, np.nan):
        dy = c["dy"].copy()
        dy[17, 2] = bad
        assert np.isnan(th.emulate_dtable(c["x"], c["table"], dy, cfg)).all()
        table = c["table"].copy()
        table[5] = bad
        assert np.isnan(th.emulate_dtable(c["x"], table, c["dy"], cfg)).all()
    off = th.offsets(cfg)
    table = c["table"].copy()
    table[off[2]:off[3]] = 0                               # an all-zero plane: every other plane's gradient is +0, its own is not
    kind, q = th.quanta(table, c["dy"], cfg, 50)
    assert kind == "sum" and [v is None for v in q[0]] == [True, True, False, True, True, True]
    d = th.emulate_dtable(c["x"], table, c["dy"], cfg)
    assert d[off[2]:off[3]].any() and not d[:off[2]].any() and not d[off[3]:].any()
    one = th.Cfg(3, 4, ((2, 2, 2),), True)
    kind, q = th.quanta(np.full(th.total(one), 3.0, np.float32), np.array([[0.75, -3.0, 0, 0]], np.float32), one, 1000)
    assert kind == "sum" and q == [[62 - 12 - (4 + 2)] * 3]    # Bnd = 3 * 3 * 3 = 27: ilogb 4; 4 N = 4000 <= 2^12
    four = th.Cfg(4, 4, ((2, 2, 2, 2),), True)
    kind, q = th.quanta(np.full(th.total(four), 2.0 ** -149, np.float32), np.full((1, 4), 2.0 ** -149, np.float32), four, 1)
    assert q == [[952] * 6]                                 # the smallest Bnd there is, 2^-894, and the smallest B: the largest q
    big = np.float32(3.4028234663852886e38)
    kind, q = th.quanta(np.full(th.total(four), big, np.float32), np.full((1, 4), big, np.float32), four, 2 ** 31 - 1)
    assert q == [[62 - 33 - (767 + 2)] * 6]                 # the largest Bnd, just below 2^768, and the largest B: the smallest q


# ---- the Python surface refuses before any kernel or library call ------------------------------------------------------------------
def test_python_refusals_without_a_device():
    import fused_hexplane as fh
    for kw, exc, word in [(dict(in_dim=2), ValueError, "in_dim must lie in 3..4"), (dict(in_dim=5), ValueError, "in_dim"),
                          (dict(in_dim=3.0), TypeError, "in_dim must be an int"), (dict(channels=0), ValueError, "channels must lie in 4..64"),
                          (dict(channels=6), ValueError, "multiple of 4"), (dict(channels=68), ValueError, "channels"),
                          (dict(channels=True), TypeError, "channels must be an int"), (dict(res=((4, 4, 4),)), ValueError, "4 resolutions"),
                          (dict(res=()), ValueError, "levels"), (dict(res=((4, 4, 4, 4),) * 9), ValueError, "levels"),
                          (dict(res=((4, 4, 1, 4),)), ValueError, "a resolution must lie in 2..4096"),
                          (dict(res=((4, 4, 4097, 4),)), ValueError, "a resolution"), (dict(res=((4, 4, 4.0, 4),)), TypeError, "a resolution must be an int"),
                          (dict(res=(4, 4, 4, 4)), TypeError, "sequence")]:
        with pytest.raises(exc, match=word):
            fh.HexPlaneConfig(**kw)
    cfg = fh.HexPlaneConfig(4, 8, ((3, 5, 4, 2),))
    total = cfg.total()
    x, table = torch.zeros((10, 4)), torch.zeros(total)
    for call in (lambda *a: fh.hex_plane(*a), lambda x, t, c: fh.hex_plane_and_grads(x, t, None, c)):
        with pytest.raises(TypeError, match="x must be a tensor"):
            call(x.numpy(), table, cfg)
        with pytest.raises(TypeError, match="table must be a tensor"):
            call(x, None, cfg)
        with pytest.raises(TypeError, match="cfg must be a HexPlaneConfig"):
            call(x, table, (4, 8))
        with pytest.raises(RuntimeError, match="x must have two dimensions"):
            call(x[0], table, cfg)
        with pytest.raises(RuntimeError, match="x must be float32"):
            call(x.double(), table, cfg)
        with pytest.raises(RuntimeError, match="table must be float32"):
            call(x, table.half(), cfg)
        with pytest.raises(ValueError, match="x must have 4 columns"):
            call(x[:, :3], table, cfg)
        with pytest.raises(RuntimeError, match=f"one flat tensor of {total} elements"):
            call(x, table[:-4], cfg)
        with pytest.raises(RuntimeError, match="one flat tensor"):
            call(x, table.view(-1, 8), cfg)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(x, table, cfg)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fh.plane_regularizer(table, cfg, tv_space=1.0)
    with pytest.raises(TypeError, match="tv_time must be"):
        fh.plane_regularizer(table, cfg, tv_time="1")
    with pytest.raises(RuntimeError, match="one flat tensor"):
        fh.plane_regularizer(table[1:], cfg)
    for kw, exc, word in [(dict(in_dim=5), ValueError, "in_dim"), (dict(channels=7), ValueError, "multiple of 4"), (dict(base=(64, 64, 64)), ValueError, "base must give 4"),
                          (dict(multires=(0,)), ValueError, "multires"), (dict(multires=(1, 128)), ValueError, "a resolution"),
                          (dict(aabb=((0, 0, 0), (1, 1, 0))), ValueError, "aabb"), (dict(aabb=((0,) * 5, (1,) * 5)), ValueError, "aabb")]:
        with pytest.raises(exc, match=word):
            fh.HexPlane(**kw)


def test_module_without_a_device():
    import fused_hexplane as fh
    m = fh.HexPlane(4, channels=8, base=(6, 5, 4, 3), multires=(1, 2), aabb=((-2, -2, -2), (2, 2, 6)))
    assert m.cfg.res == ((6, 5, 4, 3), (12, 10, 8, 3)) and m.out_dim == 16 and fh.HexPlane(3, 4, (4, 4, 4), (1,), concat=False).out_dim == 4
    assert [p is m.table for p in m.parameters()] == [True] and m.table.dtype == torch.float32 and tuple(m.table.shape) == (m.cfg.total(),)
    grids = fh.unpack_planes(m.table.detach(), m.cfg)
    for level in grids:
        for (a, b), g in zip(m.cfg.planes, level):
            if b == 3:
                assert bool((g == 1).all())                                  # the time planes start at one
            else:
                assert 0.1 <= float(g.min()) and float(g.max()) <= 0.5 and float(g.std()) > 0.05
    assert torch.equal(m.aabb_min, torch.tensor([-2.0, -2.0, -2.0])) and torch.equal(m.aabb_scale, torch.tensor([0.5, 0.5, 0.25]))
    assert "floats=" in repr(m) and fh.HexPlane().cfg.res == ((64, 64, 64, 25), (128, 128, 128, 25))
    assert fh.HexPlaneConfig(4, 8, ((3, 5, 4, 2),)) == fh.HexPlaneConfig(4, 8, [[3, 5, 4, 2]]) and fh.HexPlaneConfig(3).res == ((64, 64, 64), (128, 128, 128))


def test_the_regulariser_reference_is_k_planes():
    """(d) on a plane small enough to write out by hand"""
    c = th.Cfg(4, 4, ((2, 2, 2, 3),), True)
    rng = np.random.default_rng(1)
    table = torch.from_numpy(rng.standard_normal(th.total(c)))
    g = th.unpack(table, c)[0][2][0]                        # plane (0, 3): (C, 3, 2), time the slow axis
    tv = 2 * (((g[:, 1:] - g[:, :-1]) ** 2).sum() / (2 * 2 * 4) + ((g[:, :, 1:] - g[:, :, :-1]) ** 2).sum() / (3 * 1 * 4))
    sm = ((g[:, 2] - 2 * g[:, 1] + g[:, 0]) ** 2).mean()
    l1 = (1 - g).abs().mean()
    only = lambda **kw: float(th.regularizer_torch(table, c._replace(res=c.res), **kw))
    others = [th.unpack(table, c)[0][k][0] for k in (4, 5)]
    tvs = [2 * (((h[:, 1:] - h[:, :-1]) ** 2).sum() / (2 * 2 * 4) + ((h[:, :, 1:] - h[:, :, :-1]) ** 2).sum() / (3 * 1 * 4)) for h in others]
    assert abs(only(tv_time=1.0) - float(tv + sum(tvs))) < 1e-12
    assert abs(only(smooth_time=1.0) - float(sm + sum(((h[:, 2] - 2 * h[:, 1] + h[:, 0]) ** 2).mean() for h in others))) < 1e-12
    assert abs(only(l1_time=1.0) - float(l1 + sum((1 - h).abs().mean() for h in others))) < 1e-12
    assert only(smooth_space=1.0) == 0.0 and only(tv_space=1.0) > 0   # res_b = 2: no second difference


# ---- the kernels' resource usage ---------------------------------------------------------------------------------------------------
def test_every_kernel_compiles_without_scratch():
    """One device-only compile of hexplane.hip with the Makefile's flags: every kernel, every instantiation, 0 bytes of scratch"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^hexplane\.o: hexplane\.hip \$\(HDRS\)\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\)", mk, flags=re.M), "hexplane.o must be built with $(EXACT)"
    assert len(re.findall(r"\$\(filter \S+,[a-z0-9_ ]*\bhexplane\b[a-z0-9_ ]*\),\$\(EXACT\)", mk)) == 2, "make variant and make audit must compile hexplane uncontracted"
    assert re.search(r"^OBJS\s*:=.*\bhexplane\.o\b", mk, flags=re.M)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "hexplane.hip", "-o", os.devnull], cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == 14, names   # two maxima, prepare, convert, two of the regulariser, and D = 3, 4 of forward, dx, direct and LDS
    for kind in ("forward_kernel", "dx_kernel", "grad_direct_kernel", "grad_lds_kernel"):
        assert sum(kind in n for n in names) == 2, kind
    assert all(v == 0 for v in scratch), dict(zip(names, scratch))
