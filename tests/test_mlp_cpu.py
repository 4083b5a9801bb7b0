"""CPU: the fused MLP (include/gsr_mlp.h, fused_mlp) without a device.  The header is C99, the library exports its names and refuses
bad arguments before any device work with a text that names the function; the Python surface refuses what it must with no GPU
present; from_sequential / to_sequential round-trip; mlp.hip compiles for gfx950 with 0 bytes of scratch in every kernel.  The
references of tests/torch_mlp.py are checked against themselves: the hand-written backward rule equals autograd through mlp_ref, the
float32 chain emulation equals an exact rational evaluation and flags the midpoints it cannot decide, and the fixtures of the GPU
tests keep what they promise -- integer cases stay below 2^24 everywhere, general cases have at most 0.1 % undecided outputs and 1 %
fragile rows -- from the references alone."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import torch_mlp as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsr_mlp.h")
CSRC = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "csrc")
LIB = os.path.join(ROOT, "gaussian-splatting_cc-comments_amd", "libgsr_hip.so")
NAMES = ["gsr_mlp_backward", "gsr_mlp_forward", "gsr_mlp_scratch_bytes", "gsr_mlp_tile_rows"]


def _lib():
    if not os.path.exists(LIB):
        __graft_entry__.build()
    import fused_mlp
    L = fused_mlp._lib()
    L.gsr_last_error.restype = ctypes.c_char_p
    return L


def _desc(N=10, widths=(3, 16, 2), D=None, L=0, hidden=1, out=0, xl=0, yl=0, xs=None, ys=None, dys=None, dxs=None, wg=0):
    import fused_mlp
    d = fused_mlp.MlpDesc(N=N, M=len(widths) - 1, D=widths[0] if D is None else D, L=L, hidden_activation=hidden, output_activation=out,
                          x_layout=xl, y_layout=yl, max_workgroups=wg)
    for l, w in enumerate(widths):
        d.widths[l] = w
    d.x_stride = (N if xl else d.D) if xs is None else xs
    d.y_stride = (N if yl else widths[-1]) if ys is None else ys
    d.dy_stride = d.y_stride if dys is None else dys
    d.dx_stride = d.x_stride if dxs is None else dxs
    return d


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_is_c99(tmp_path):
    src = tmp_path / "use_mlp.c"
    src.write_text('#include "gsr_mlp.h"\n#include "gsr_mlp.h"\n'
                   "int use(void) { gsr_mlp_desc d; d.N = 0; return (int)(sizeof(&gsr_mlp_forward) + sizeof(&gsr_mlp_backward) + sizeof d) + "
                   "GSR_MLP_MAX_WIDTH + GSR_MLP_PLANES + GSR_MLP_TANH + d.N; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "use_mlp.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_library_exports_the_names_of_the_header():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr))) == NAMES
    L = _lib()
    for n in NAMES:
        assert hasattr(L, n), n


def test_the_record_is_the_headers():
    import fused_mlp
    assert ctypes.sizeof(fused_mlp.MlpDesc) == 4 * 2 + 4 * 6 + 4 * 6 + 8 * 4 + 8   # ints, widths, ints, strides, max_workgroups + padding
    assert fused_mlp.MlpDesc.x_stride.offset == 56 and fused_mlp.MlpDesc.max_workgroups.offset == 88


def test_entry_points_refuse_before_any_device_work():
    L = _lib()
    p = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused or has nothing to do
    ptrs = (ctypes.c_void_p * 5)(4096, 4096, 4096, 4096, 4096)

    def fwd(word, d=None, x=p, w=ptrs, b=None, y=p, scratch=p):
        d = _desc() if d is None else d
        assert L.gsr_mlp_forward(ctypes.byref(d) if d is not False else None, x, w, b, y, scratch, None) == -1, word
        text = L.gsr_last_error().decode()
        assert text.startswith("gsr_mlp_forward:") and word in text, text

    def bwd(word, d=None, x=p, w=ptrs, dy=p, dx=p, scratch=p):
        d = _desc() if d is None else d
        assert L.gsr_mlp_backward(ctypes.byref(d), x, w, None, dy, dx, None, None, scratch, None) == -1, word
        text = L.gsr_last_error().decode()
        assert text.startswith("gsr_mlp_backward:") and word in text, text

    fwd("desc is NULL", d=False)
    fwd("negative count", _desc(N=-1))
    fwd("M must lie in 1..5", _desc(widths=(3,)))
    d6 = _desc()
    d6.M = 6
    fwd("M must lie in 1..5", d6)
    fwd("widths[1] must lie in 1..128", _desc(widths=(3, 129, 2)))
    fwd("widths[2] must lie in 1..128", _desc(widths=(3, 16, 0)))
    fwd("L must lie in 0..10", _desc(L=11, D=3))
    fwd("L must lie in 0..10", _desc(L=-1, D=3))
    fwd("widths[0] must be D (1 + 2 L)", _desc(widths=(10, 16, 2), D=3, L=1))
    fwd("widths[0] must be D (1 + 2 L)", _desc(D=0))
    fwd("unknown hidden activation", _desc(hidden=2))
    fwd("unknown output activation", _desc(out=1))
    fwd("unknown layout", _desc(xl=2))
    fwd("unknown layout", _desc(yl=-1))
    fwd("negative max_workgroups", _desc(wg=-1))
    fwd("stride is smaller", _desc(xs=2))
    fwd("stride is smaller", _desc(ys=1))
    fwd("stride is smaller", _desc(xl=1, xs=9))
    fwd("stride is smaller", _desc(yl=1, ys=9))
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(scratch=None)):
        fwd("is NULL", **kw)
    fwd("weights[1] is NULL", w=(ctypes.c_void_p * 5)(4096, None, 4096, 4096, 4096))
    fwd("16-byte aligned", scratch=ctypes.c_void_p(4100))
    bwd("negative count", _desc(N=-1))
    bwd("stride is smaller", _desc(dys=1))
    bwd("stride is smaller", _desc(dxs=2))
    bwd("is NULL", dy=None)
    bwd("16-byte aligned", scratch=ctypes.c_void_p(4104))
    d0 = _desc(N=0)
    assert L.gsr_mlp_forward(ctypes.byref(d0), None, None, None, None, None, None) == 0   # nothing to do, whatever the pointers
    assert L.gsr_mlp_backward(ctypes.byref(d0), None, None, None, None, None, None, None, None, None) == 0


def test_scratch_and_tile_rows():
    L = _lib()
    s, r = L.gsr_mlp_scratch_bytes, L.gsr_mlp_tile_rows
    for bad in (_desc(N=-1), _desc(widths=(3, 129, 2)), _desc(L=11, D=3), _desc(D=2)):
        assert s(ctypes.byref(bad)) == 0 and r(ctypes.byref(bad)) == 0
    assert s(None) == 0 and r(None) == 0
    small, wide = _desc(N=1000, widths=(3, 16, 2)), _desc(N=1000, widths=(128,) * 6)
    assert s(ctypes.byref(small)) > 0 and s(ctypes.byref(small)) % 16 == 0 and s(ctypes.byref(wide)) > s(ctypes.byref(small))
    # the partials grow with the workgroups, never with N beyond them: nothing of size N x width
    assert s(ctypes.byref(_desc(N=6000000, widths=(64, 64, 64, 3)))) == s(ctypes.byref(_desc(N=600000, widths=(64, 64, 64, 3))))
    assert s(ctypes.byref(_desc(N=6000000, widths=(64, 64, 64, 3)))) < 64 << 20
    assert s(ctypes.byref(_desc(N=1000, wg=1))) < s(ctypes.byref(_desc(N=1000, wg=3)))
    # R is a function of the widths alone, a power of two between 16 and 128, smaller for wide and deep networks
    rows = {w: r(ctypes.byref(_desc(N=n, widths=w))) for w in ((3, 16, 2), (64, 64, 64, 3), (128,) * 6) for n in (1, 100000)}
    assert rows[(3, 16, 2)] == 128 and rows[(128,) * 6] == 16 and rows[(64, 64, 64, 3)] in (32, 64, 128)
    for w in ((3, 16, 2), (64, 64, 64, 3), (128,) * 6):
        assert r(ctypes.byref(_desc(N=1, widths=w))) == r(ctypes.byref(_desc(N=100000, widths=w, wg=7)))


def test_every_kernel_compiles_without_scratch():
    """One device-only compile of mlp.hip with the Makefile's flags: every kernel, every instantiation, 0 bytes of scratch"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^mlp\.o: mlp\.hip \$\(HDRS\)\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\)", mk, flags=re.M), "mlp.o must be built with $(EXACT)"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "mlp.hip", "-o", os.devnull], cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == 10, names   # prepare, fold, four forward and four backward instantiations
    assert sum("forward_kernel" in n for n in names) == 4 and sum("backward_kernel" in n for n in names) == 4
    assert all(v == 0 for v in scratch), dict(zip(names, scratch))


# ---- the Python surface refuses before any kernel or library call ------------------------------------------------------------------
def test_python_refusals_without_a_device():
    import fused_mlp as fm
    x = torch.zeros((10, 3))
    W = [torch.zeros((16, 3)), torch.zeros((2, 16))]
    with pytest.raises(TypeError):
        fm.mlp(x.numpy(), W)
    with pytest.raises(TypeError):
        fm.mlp(x, [W[0].numpy(), W[1]])
    with pytest.raises(TypeError):
        fm.mlp(x, W, activation=1)
    with pytest.raises(TypeError):
        fm.mlp(x, W, frequencies=1.0)
    with pytest.raises(TypeError):
        fm.mlp(x, W, [torch.zeros(16), 3.0])
    with pytest.raises(ValueError, match="activation must be one of"):
        fm.mlp(x, W, activation="gelu")
    with pytest.raises(ValueError, match="output_activation must be one of"):
        fm.mlp(x, W, output_activation="relu")
    with pytest.raises(ValueError, match="layout must be one of"):
        fm.mlp(x, W, layout="cols")
    with pytest.raises(ValueError, match="out_layout must be one of"):
        fm.mlp(x, W, out_layout="cols")
    with pytest.raises(ValueError, match="frequencies must lie in 0..10"):
        fm.mlp(x, W, frequencies=11)
    with pytest.raises(ValueError, match="1..5 tensors"):
        fm.mlp(x, [])
    with pytest.raises(ValueError, match="1..5 tensors"):
        fm.mlp(x, [W[0]] * 6)
    with pytest.raises(ValueError, match="one entry"):
        fm.mlp(x, W, [None])
    with pytest.raises(RuntimeError, match="float32"):
        fm.mlp(x.double(), W)
    with pytest.raises(RuntimeError, match="two dimensions"):
        fm.mlp(x[0], W)
    with pytest.raises(RuntimeError, match="must have 3 columns"):
        fm.mlp(x, [torch.zeros((16, 4)), W[1]])
    with pytest.raises(RuntimeError, match="must have 9 columns"):
        fm.mlp(x, W, frequencies=1)
    with pytest.raises(RuntimeError, match="must have 16 columns"):
        fm.mlp(x, [W[0], torch.zeros((2, 15))])
    with pytest.raises(ValueError, match="1..128 rows"):
        fm.mlp(x, [torch.zeros((129, 3))])
    with pytest.raises(ValueError, match="1..128 columns after the encoding"):
        fm.mlp(torch.zeros((10, 7)), [torch.zeros((4, 147))], frequencies=10)
    with pytest.raises(RuntimeError, match=r"biases\[0\] must be float32 of shape \(16,\)"):
        fm.mlp(x, W, [torch.zeros(15), None])
    with pytest.raises(RuntimeError, match="no CPU path"):
        fm.mlp(x, W)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fm.mlp_and_grads(x, W, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fm.TinyMLP(3, 2)(x)
    with pytest.raises(ValueError):
        fm.TinyMLP(3, 2, hidden=129)
    with pytest.raises(ValueError):
        fm.TinyMLP(3, 2, hidden_layers=5)
    with pytest.raises(ValueError, match="at most 128 columns"):
        fm.TinyMLP(7, 2, frequencies=10)
    with pytest.raises(TypeError):
        fm.decode_feature_map(torch.zeros((3, 4, 5)), torch.nn.Linear(3, 2))
    with pytest.raises(RuntimeError, match=r"\(K, H, W\)"):
        fm.decode_feature_map(torch.zeros((3, 4)), fm.TinyMLP(3, 2))
    with pytest.raises(RuntimeError, match="4 channels"):
        fm.decode_feature_map(torch.zeros((4, 4, 5)), fm.TinyMLP(3, 2))


def test_sequential_round_trip():
    import fused_mlp as fm
    torch.manual_seed(5)
    nn = torch.nn
    seq = nn.Sequential(nn.Linear(7, 33), nn.ReLU(), nn.Linear(33, 20), nn.ReLU(), nn.Identity(), nn.Linear(20, 3), nn.Sigmoid())
    m = fm.TinyMLP.from_sequential(seq)
    assert (m.in_dim, m.out_dim, m.frequencies, m.activation, m.output_activation) == (7, 3, 0, "relu", "sigmoid")
    assert [tuple(w.shape) for w in m.weights] == [(33, 7), (20, 33), (3, 20)]
    back = m.to_sequential()
    assert [type(a) for a in back] == [type(a) for a in seq if not isinstance(a, nn.Identity)]
    x = torch.randn(50, 7)
    assert torch.equal(back(x), seq(x))                       # clones of the same bits through the same modules
    assert m.weights[0].data_ptr() != seq[0].weight.data_ptr()
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    assert sorted(m.state_dict()) == ["biases.0", "biases.1", "biases.2", "weights.0", "weights.1", "weights.2"]
    assert len(list(m.parameters())) == 6 and all(p.dtype == torch.float32 and p.is_contiguous() for p in m.parameters())
    # an encoding in front, no ReLU, no bias, tanh
    seq2 = nn.Sequential(fm.FrequencyEncoding(2), nn.Linear(15, 8, bias=False), nn.Linear(8, 4, bias=False), nn.Tanh())
    m2 = fm.TinyMLP.from_sequential(seq2)
    assert (m2.in_dim, m2.frequencies, m2.activation, m2.output_activation, m2.biases) == (3, 2, "none", "tanh", None)
    x3 = torch.randn(9, 3)
    assert torch.equal(m2.to_sequential()(x3), seq2(x3))
    enc = fm.FrequencyEncoding(2)(x3)
    assert torch.equal(enc[:, 3:6], torch.sin(x3)) and torch.equal(enc[:, 12:15], torch.cos(2 * x3))
    # the stock initialisation and shapes of the constructor
    m3 = fm.TinyMLP(4, 3, hidden=64, hidden_layers=2, frequencies=10)
    assert [tuple(w.shape) for w in m3.weights] == [(64, 84), (64, 64), (3, 64)] and len(m3.to_sequential()) == 6
    for bad in (nn.Sequential(nn.ReLU()), nn.Sequential(nn.Linear(3, 4), nn.ReLU(), nn.ReLU(), nn.Linear(4, 2)),
                nn.Sequential(nn.Linear(3, 4), nn.Linear(4, 4), nn.ReLU(), nn.Linear(4, 2)), nn.Sequential(nn.Linear(3, 4), nn.GELU(), nn.Linear(4, 2)),
                nn.Sequential(nn.Linear(3, 4), nn.ReLU(), nn.Linear(4, 2, bias=False)), nn.Sequential(fm.FrequencyEncoding(1), nn.Linear(4, 2))):
        with pytest.raises(ValueError, match="from_sequential"):
            fm.TinyMLP.from_sequential(bad)


# ---- the references against themselves ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [0, 1, 10])
@pytest.mark.parametrize("act,outa", [("relu", "none"), ("relu", "sigmoid"), ("none", "tanh"), ("relu", "tanh")])
def test_backward_rule_equals_autograd(L, act, outa):
    g = torch.Generator().manual_seed(100 + L)
    D, widths = 3, [3 * (1 + 2 * L), 17, 9, 4]
    x = torch.randn(41, D, generator=g, dtype=torch.float64) * (0.01 if L == 10 else 1.0)
    Ws = [torch.randn(widths[l + 1], widths[l], generator=g, dtype=torch.float64) / widths[l] ** 0.5 for l in range(3)]
    bs = [torch.randn(widths[l + 1], generator=g, dtype=torch.float64) for l in range(3)]
    dy = torch.randn(41, 4, generator=g, dtype=torch.float64)
    leaves = [t.requires_grad_(True) for t in [x] + Ws + bs]
    (tm.mlp_ref(x, Ws, bs, act, outa, L) * dy).sum().backward()
    auto = [t.grad for t in leaves]
    with torch.no_grad():
        for drop in (None, "dx", "dW", "db"):
            dx, dW, db = tm.backward_ref(x, Ws, bs, dy, act, outa, L, want_dx=drop != "dx", want_dw=drop != "dW", want_db=drop != "db")
            assert (dx is None) == (drop == "dx") and (dW is None) == (drop == "dW") and (db is None) == (drop == "db")
            mine = [dx] + (dW or [None] * 3) + (db or [None] * 3)
            for k, (a, b) in enumerate(zip(mine, auto)):
                if a is None:
                    continue
                scale = b.abs().max().clamp_min(1.0) * (2.0 ** L)   # the terms' moduli: the encoding's chain rule multiplies by up to 2^(L-1)
                assert (a - b).abs().max() <= 1e-12 * scale, (drop, k, float((a - b).abs().max()))


def _round_f32(fr):
    """A Fraction, rounded once to the nearest float32 (ties to even); normal range only"""
    if fr == 0:
        return np.float32(0)
    sgn, fr = (-1, -fr) if fr < 0 else (1, fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    assert Fraction(2) ** e <= fr < Fraction(2) ** (e + 1) and -120 < e < 120
    q = fr / Fraction(2) ** (e - 23)
    n, rem = divmod(q.numerator, q.denominator)
    twice = 2 * rem
    if twice > q.denominator or (twice == q.denominator and n & 1):
        n += 1
    return np.float32(sgn * float(Fraction(n) * Fraction(2) ** (e - 23)))   # exact: n has at most 25 bits


def test_chain_emulation_is_exact_where_it_says_so():
    rng = np.random.default_rng(12)
    w = rng.standard_normal(300).astype(np.float32)
    a = rng.standard_normal(300).astype(np.float32)
    acc = (rng.standard_normal(300) * 10.0 ** rng.integers(-3, 3, 300)).astype(np.float32)
    # constructed cases.  The exact sum IS a float32 midpoint, a true tie that both roundings break to even: decided, and equal ...
    w = np.concatenate([w, np.float32([2.0 ** -12, 2.0 ** -12, -2.0 ** -12, 2.0 ** -11])])
    a = np.concatenate([a, np.float32([2.0 ** -12, 3 * 2.0 ** -12, 2.0 ** -12, 2.0 ** -11])])
    acc = np.concatenate([acc, np.float32([1.0, 1.0, 2.0, 4.0])])   # 1 + 2^-24, 1 + 3 2^-24, 2 - 2^-24, 4 + 2^-22
    # ... but a sum that float64 rounds ONTO a midpoint must be flagged.  From just below it: (1 + 2^-23 + 2^-24) - 2^-70, which fmaf
    # rounds down to 1 + 2^-23 and the two-step rounding, from the tie, up to the even 1 + 2^-22.  From just above it:
    # (1 + 2^-24) + 2^-70, which fmaf rounds up to 1 + 2^-23 and the two-step rounding down to the even 1.
    w = np.concatenate([w, np.float32([2.0 ** -12 * (1 + 2.0 ** -23), 2.0 ** -12 * (1 + 2.0 ** -23)])])
    a = np.concatenate([a, np.float32([2.0 ** -12 * (1 - 2.0 ** -23), -2.0 ** -12 * (1 - 2.0 ** -23)])])
    acc = np.concatenate([acc, np.float32([1 + 2.0 ** -23, 1 + 2.0 ** -23])])
    got, und = tm.fma_fp32(w, a, acc)
    exact = np.array([_round_f32(Fraction(float(wi)) * Fraction(float(ai)) + Fraction(float(ci))) for wi, ai, ci in zip(w, a, acc)], np.float32)
    assert und[304:].all() and not und[:304].any(), und[300:]
    assert got[304] != exact[304] and got[305] != exact[305]   # the cases the flag exists for
    assert np.array_equal(got[~und], exact[~und])
    # the chain: the same against rationals, and the flag sticks to the element from the step it was raised
    W = rng.standard_normal((5, 9)).astype(np.float32)
    A = rng.standard_normal((4, 9)).astype(np.float32)
    b = rng.standard_normal(5).astype(np.float32)
    z, und = tm.chain_fp32(W, A, b)
    for n in range(4):
        for o in range(5):
            acc1 = np.float32(b[o])
            for k in range(9):
                acc1 = _round_f32(Fraction(float(W[o, k])) * Fraction(float(A[n, k])) + Fraction(float(acc1)))
            assert z[n, o] == acc1 and not und[n, o]
    W[2, 3], A[1, 3], W[2, :3], W[2, 4:] = 2.0 ** -12 * (1 + 2.0 ** -23), 2.0 ** -12 * (1 - 2.0 ** -23), 0, 0
    b[2] = 1 + 2.0 ** -23
    z, und = tm.chain_fp32(W, A, b)
    assert und[1, 2] and und.sum() == 1


@pytest.mark.parametrize("name", sorted(tm.INTEGER_SHAPES))
@pytest.mark.parametrize("asymmetric", [False, True])
def test_integer_fixtures_are_exact_in_float32(name, asymmetric):
    """Weights in {-1, 0, 1} (distinct small integers in the asymmetric form), bounded fan-in; every partial sum of the forward, of the
    backward and of dW and db over all rows -- bounded by the computation on moduli -- stays below 2^24."""
    c = tm.integer_fixture(name, asymmetric)
    for arr in [c["x"], c["dy"]] + c["Ws"] + (c["bs"] or []):
        assert np.array_equal(arr, np.round(arr)) and np.abs(arr).max() <= 3
    if asymmetric:
        for l, W in enumerate(c["Ws"], 1):
            assert all(np.flatnonzero(W[o]).tolist() == [(o + l) % W.shape[1]] for o in range(W.shape[0]))
            assert len(set(W[W != 0].tolist())) == min(3, W.shape[0])
    else:
        assert all((W != 0).sum(1).max() <= 6 and (W != 0).sum(0).max() <= 6 for W in c["Ws"])
    x, Ws, bs, dy = tm.t64(c)
    _, zabs = tm.mlp_ref(x, Ws, bs, absolute=True, layers=True)
    assert max(float(z.max()) for z in zabs) < 2 ** 24
    ax, aW, ab = tm.backward_ref(x.abs(), [W.abs() for W in Ws], None if bs is None else [b.abs() for b in bs], dy.abs(), "none", "none", 0)
    assert max(float(t.max()) for t in [ax] + aW + ab) < 2 ** 24


@pytest.mark.parametrize("name", sorted(tm.GENERAL_SHAPES))
def test_general_fixtures_are_decided_and_robust(name):
    c = tm.general_fixture(name)
    em = tm.emulate(c["x"], c["Ws"], c["bs"], c["dy"])
    _, und = tm.chain_fp32(c["Ws"][-1], em["a"][-1], c["bs"][-1])
    assert em["undecided"].mean() <= 0.001 and und.mean() <= 0.001, (em["undecided"].mean(), und.mean())
    x, Ws, bs, dy = tm.t64(c)
    b = tm.bars(x, Ws, bs, dy)
    assert float(b["fragile"].double().mean()) <= 0.01, float(b["fragile"].double().mean())
    # the emulation lies within the float64 check's own bars: the two references agree with each other
    y64 = tm.mlp_ref(x, Ws, bs)
    assert bool((torch.from_numpy(em["z"].astype(np.float64)) - y64).abs().le(b["y"]).all())


@pytest.mark.parametrize("L,D", sorted(tm.ENCODED_SEEDS))
def test_encoded_fixtures_are_robust(L, D):
    c = tm.encoded_fixture(L, D)
    x, Ws, bs, dy = tm.t64(c)
    assert float(x.abs().max()) * 2.0 ** (L - 1) < 32
    b = tm.bars(x, Ws, bs, dy, L=L)
    assert float(b["fragile"].double().mean()) <= 0.01, float(b["fragile"].double().mean())
