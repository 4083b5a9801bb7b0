"""A fully fused small MLP on the fp32-input matrix cores, with an optional frequency encoding (include/gsr_mlp.h): what Scaffold-GS's
anchor decoders, Deformable-3DGS's deformation field, Compact-3DGS's colour field and per-pixel decoders of rendered feature maps
evaluate on every Gaussian, anchor or pixel, every step -- tiny-cuda-nn's FullyFusedMLP in float32.

    mlp(x, weights, biases, activation="relu", output_activation="none", frequencies=0, layout="rows", out_layout=None) -> y
    mlp_and_grads(x, weights, biases, dy, ...)   -> (y, dx, dW, db), the raw forward and backward calls
    TinyMLP(in_dim, out_dim, hidden=64, hidden_layers=2, ...)   an nn.Module; .from_sequential(seq) / .to_sequential()
    decode_feature_map(feature_map (K, H, W), mlp) -> (C, H, W), reading the rasterizer's feature_map in place

    dec = TinyMLP(32, 3, hidden=64, hidden_layers=2, output_activation="sigmoid").cuda()
    color, radii, fmap = GaussianRasterizer(settings)(..., features=f)
    rgb = decode_feature_map(fmap, dec)          # gradients reach dec's parameters, f, and every Gaussian input

weights[l] is (d_{l+1}, d_l) as nn.Linear's, biases[l] (d_{l+1},) or None.  layout "rows": x is (N, D), any row stride; "planes": x is
(D, N), which is what feature_map.view(K, H * W) is.  With frequencies = L the first layer is d_0 = D (1 + 2 L) wide and reads
(x, sin(2^0 x), cos(2^0 x), ..), which is never stored.  Every layer is one float32 fmaf chain in ascending input order, started at
the bias; nothing of size N x hidden is written, the forward saves nothing (the backward recomputes it from x), dW and db are summed
in an order fixed by N and the widths: every result has the same bits every run.  HIP tensors only (no CPU path)."""
import ctypes

import torch

from diff_gaussian_rasterization import _binding

MAX_LAYERS = 5      # include/gsr_mlp.h GSR_MLP_MAX_LAYERS
MAX_WIDTH = 128     # GSR_MLP_MAX_WIDTH
MAX_OCTAVES = 10    # GSR_MLP_MAX_OCTAVES
_HIDDEN = {"none": 0, "relu": 1}
_OUTPUT = {"none": 0, "sigmoid": 2, "tanh": 3}
_LAYOUT = {"rows": 0, "planes": 1}


class MlpDesc(ctypes.Structure):
    """gsr_mlp_desc"""
    _fields_ = [("N", ctypes.c_int), ("M", ctypes.c_int), ("widths", ctypes.c_int * (MAX_LAYERS + 1)), ("D", ctypes.c_int),
                ("L", ctypes.c_int), ("hidden_activation", ctypes.c_int), ("output_activation", ctypes.c_int),
                ("x_layout", ctypes.c_int), ("y_layout", ctypes.c_int), ("x_stride", ctypes.c_longlong),
                ("y_stride", ctypes.c_longlong), ("dy_stride", ctypes.c_longlong), ("dx_stride", ctypes.c_longlong),
                ("max_workgroups", ctypes.c_int)]


_vp, _dp = ctypes.c_void_p, ctypes.POINTER(MlpDesc)
_lib, _run = _binding.declare("gsr_mlp.h", {
    "gsr_mlp_tile_rows": (ctypes.c_int, [_dp]),
    "gsr_mlp_scratch_bytes": (ctypes.c_size_t, [_dp]),
    "gsr_mlp_forward": (ctypes.c_int, [_dp] + [_vp] * 6),
    "gsr_mlp_backward": (ctypes.c_int, [_dp] + [_vp] * 9),
}, {"gsr_mlp_desc": MlpDesc})
_pointers, _check_int, _check_matrix, _strided, _stride0 = (
    _binding.pointers, _binding.check_int, _binding.check_matrix, _binding.strided, _binding.stride0)


def _choice(name, v, table):
    if not isinstance(v, str):
        raise TypeError(f"{name} must be one of {tuple(table)}, got {v!r}")
    if v not in table:
        raise ValueError(f"{name} must be one of {tuple(table)}, got {v!r}")
    return table[v]


def check(x, weights, biases, activation, output_activation, frequencies, layout, out_layout, max_workgroups=0):
    """Every refusal of the surface, before the library is loaded -> (MlpDesc without strides, the biases as a list)."""
    hid, outa = _choice("activation", activation, _HIDDEN), _choice("output_activation", output_activation, _OUTPUT)
    xl = _choice("layout", layout, _LAYOUT)
    yl = xl if out_layout is None else _choice("out_layout", out_layout, _LAYOUT)
    _check_int("frequencies", frequencies, 0, MAX_OCTAVES)
    _check_int("max_workgroups", max_workgroups, 0, 1 << 20)
    _check_matrix("x", x)
    if not isinstance(weights, (list, tuple)) or not 1 <= len(weights) <= MAX_LAYERS:
        raise ValueError(f"weights must be a list of 1..{MAX_LAYERS} tensors")
    M = len(weights)
    biases = [None] * M if biases is None else list(biases)
    if len(biases) != M:
        raise ValueError(f"biases must be None or hold one entry (a tensor or None) per layer: {M}; got {len(biases)}")
    N, D = (x.shape[0], x.shape[1]) if xl == 0 else (x.shape[1], x.shape[0])
    if N >= 1 << 31:
        raise ValueError(f"x must have fewer than 2^31 rows; got {N}")
    if D < 1 or D * (1 + 2 * frequencies) > MAX_WIDTH:
        raise ValueError(f"x must have 1..{MAX_WIDTH} columns after the encoding; got {D} x (1 + 2 x {frequencies})")
    width = D * (1 + 2 * frequencies)
    widths = [width]
    for l, (w, b) in enumerate(zip(weights, biases)):
        _check_matrix(f"weights[{l}]", w)
        if w.shape[1] != width:
            raise RuntimeError(f"weights[{l}] must have {width} columns (the width of its input); got {tuple(w.shape)}")
        width = int(w.shape[0])
        if not 1 <= width <= MAX_WIDTH:
            raise ValueError(f"weights[{l}] must have 1..{MAX_WIDTH} rows; got {width}")
        if b is not None:
            if not torch.is_tensor(b):
                raise TypeError(f"biases[{l}] must be a tensor or None")
            if b.dtype != torch.float32 or tuple(b.shape) != (width,):
                raise RuntimeError(f"biases[{l}] must be float32 of shape ({width},); got {b.dtype} {tuple(b.shape)}")
        widths.append(width)
    tensors = [x] + list(weights) + [b for b in biases if b is not None]
    dev = x.device
    if dev.type != "cuda" or any(t.device != dev for t in tensors):
        raise RuntimeError("the tensors must be HIP (cuda) tensors on one device; the fused MLP has no CPU path")
    d = MlpDesc(N=int(N), M=M, D=int(D), L=frequencies, hidden_activation=hid, output_activation=outa, x_layout=xl, y_layout=yl,
                max_workgroups=max_workgroups)
    for l, wd in enumerate(widths):
        d.widths[l] = wd
    return d, biases


def _prepare(x, weights, biases):
    xs = _strided(x.detach())
    ws = [w.detach().contiguous() for w in weights]
    bs = [None if b is None else b.detach().contiguous() for b in biases]
    return xs, ws, bs


def _forward(d, xs, ws, bs):
    dev = xs.device
    N, dM = d.N, d.widths[d.M]
    y = torch.empty((N, dM) if d.y_layout == 0 else (dM, N), dtype=torch.float32, device=dev)
    if N == 0:
        return y
    d.x_stride, d.y_stride = _stride0(xs), _stride0(y)
    with torch.cuda.device(dev):
        scratch = torch.empty((_lib().gsr_mlp_scratch_bytes(ctypes.byref(d)),), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        _run("gsr_mlp_forward", ctypes.byref(d), xs.data_ptr(), _pointers(ws), _pointers(bs), y.data_ptr(), scratch.data_ptr(), stream.cuda_stream)
        for t in [scratch, xs] + ws + [b for b in bs if b is not None]:
            t.record_stream(stream)
    return y


def _backward(d, xs, ws, bs, dy, want_dx, want_dw, want_db):
    """want_dw, want_db: one bool per layer -> (dx or None, [dW_l or None], [db_l or None])"""
    dev = xs.device
    dys = _strided(dy.detach())
    dx = torch.empty_like(xs, memory_format=torch.contiguous_format) if want_dx else None
    dW = [torch.empty_like(w) if k else None for w, k in zip(ws, want_dw)]
    db = [torch.empty((w.shape[0],), dtype=torch.float32, device=dev) if k else None for w, k in zip(ws, want_db)]
    d.x_stride, d.dy_stride = _stride0(xs), _stride0(dys)
    d.y_stride = d.dy_stride
    d.dx_stride = _stride0(dx) if want_dx else 0
    with torch.cuda.device(dev):
        scratch = torch.empty((max(16, _lib().gsr_mlp_scratch_bytes(ctypes.byref(d))),), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        _run("gsr_mlp_backward", ctypes.byref(d), xs.data_ptr(), _pointers(ws), _pointers(bs), dys.data_ptr(), None if dx is None else dx.data_ptr(),
             _pointers(dW), _pointers(db), scratch.data_ptr(), stream.cuda_stream)
        for t in [scratch, xs, dys] + ws + [b for b in bs if b is not None]:
            t.record_stream(stream)
    return dx, dW, db


@torch.no_grad()
def mlp_and_grads(x, weights, biases, dy=None, *, activation="relu", output_activation="none", frequencies=0, layout="rows", out_layout=None,
                  want_dx=True, want_dw=True, want_db=True, max_workgroups=0):
    """The raw calls -> (y, dx, dW, db).  dy: the gradient of y in y's layout, or None = the forward alone (dx, dW, db are then None).
    want_dw / want_db: a bool, or one per layer; what is not wanted is None in the result and is not formed.  db of a layer without a
    bias is formed all the same when wanted."""
    d, biases = check(x, weights, biases, activation, output_activation, frequencies, layout, out_layout, max_workgroups)
    xs, ws, bs = _prepare(x, weights, biases)
    y = _forward(d, xs, ws, bs)
    if dy is None:
        return y, None, None, None
    _check_matrix("dy", dy)
    if dy.shape != y.shape or dy.device != y.device:
        raise RuntimeError(f"dy must have y's shape {tuple(y.shape)} on its device; got {tuple(dy.shape)} on {dy.device}")
    per_layer = lambda v: [bool(v)] * d.M if isinstance(v, bool) else [bool(k) for k in v]
    dx, dW, db = _backward(d, xs, ws, bs, dy, bool(want_dx), per_layer(want_dw), per_layer(want_db))
    return y, dx, dW, db


class _Mlp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cfg, M, *params):
        weights, biases = params[:M], params[M:]
        d, biases = check(x, weights, biases, *cfg)
        xs, ws, bs = _prepare(x, weights, biases)
        ctx.cfg, ctx.M = cfg, M
        ctx.has_bias = [b is not None for b in bs]
        ctx.save_for_backward(xs, *ws, *[b for b in bs if b is not None])   # x and the parameters: no activation is kept
        return _forward(d, xs, ws, bs)

    @staticmethod
    def backward(ctx, dy):
        M = ctx.M
        saved = list(ctx.saved_tensors)
        xs, ws, rest = saved[0], saved[1:1 + M], saved[1 + M:]
        bs = [rest.pop(0) if h else None for h in ctx.has_bias]
        need = ctx.needs_input_grad
        want_dw = [need[3 + l] for l in range(M)]
        want_db = [need[3 + M + l] and ctx.has_bias[l] for l in range(M)]
        d, _ = check(xs, ws, bs, *ctx.cfg)
        dx, dW, db = _backward(d, xs, ws, bs, dy, need[0], want_dw, want_db)
        return (dx, None, None) + tuple(dW) + tuple(db)


def mlp(x, weights, biases=None, *, activation="relu", output_activation="none", frequencies=0, layout="rows", out_layout=None):
    """y = the network of the module docstring applied to every row of x; differentiable w.r.t. x, the weights and the biases, each
    gradient formed only where it is required (a frozen decoder, an input without a gradient)."""
    cfg = (activation, output_activation, frequencies, layout, out_layout)
    if not isinstance(weights, (list, tuple)):
        raise ValueError(f"weights must be a list of 1..{MAX_LAYERS} tensors")
    biases = [None] * len(weights) if biases is None else list(biases)
    if len(biases) != len(weights):
        raise ValueError(f"biases must be None or hold one entry (a tensor or None) per layer: {len(weights)}; got {len(biases)}")
    check(x, weights, biases, *cfg)
    return _Mlp.apply(x, cfg, len(weights), *weights, *biases)


class FrequencyEncoding(torch.nn.Module):
    """(x, sin(2^0 x), cos(2^0 x), .., sin(2^{L-1} x), cos(2^{L-1} x)) along the last dimension in torch operations: the first module
    of TinyMLP.to_sequential() when the network has an encoding."""

    def __init__(self, frequencies):
        super().__init__()
        _check_int("frequencies", frequencies, 1, MAX_OCTAVES)
        self.frequencies = frequencies

    def forward(self, x):
        out = [x]
        for j in range(self.frequencies):
            out += [torch.sin(x * 2.0 ** j), torch.cos(x * 2.0 ** j)]
        return torch.cat(out, dim=-1)


class TinyMLP(torch.nn.Module):
    """in_dim -> hidden x hidden_layers -> out_dim with nn.Linear's parameters, layouts and initialisation, evaluated by mlp().
    .weights and .biases are ParameterLists of float32 tensors: list(module.parameters()) is one FusedAdam group.
    forward(x, layout="rows", out_layout=None): x (N, in_dim), or (in_dim, N) with layout="planes"."""

    def __init__(self, in_dim, out_dim, hidden=64, hidden_layers=2, activation="relu", output_activation="none", frequencies=0, bias=True):
        super().__init__()
        _check_int("in_dim", in_dim, 1, MAX_WIDTH)
        _check_int("out_dim", out_dim, 1, MAX_WIDTH)
        _check_int("hidden", hidden, 1, MAX_WIDTH)
        _check_int("hidden_layers", hidden_layers, 0, MAX_LAYERS - 1)
        _check_int("frequencies", frequencies, 0, MAX_OCTAVES)
        _choice("activation", activation, _HIDDEN)
        _choice("output_activation", output_activation, _OUTPUT)
        if in_dim * (1 + 2 * frequencies) > MAX_WIDTH:
            raise ValueError(f"the encoded input must have at most {MAX_WIDTH} columns; got {in_dim} x (1 + 2 x {frequencies})")
        self.in_dim, self.out_dim, self.frequencies = in_dim, out_dim, frequencies
        self.activation, self.output_activation = activation, output_activation
        widths = [in_dim * (1 + 2 * frequencies)] + [hidden] * hidden_layers + [out_dim]
        layers = [torch.nn.Linear(a, b, bias=bias) for a, b in zip(widths[:-1], widths[1:])]   # nn.Linear's initialisation
        self.weights = torch.nn.ParameterList([l.weight for l in layers])
        self.biases = torch.nn.ParameterList([l.bias for l in layers]) if bias else None

    def forward(self, x, layout="rows", out_layout=None):
        return mlp(x, list(self.weights), None if self.biases is None else list(self.biases), activation=self.activation,
                   output_activation=self.output_activation, frequencies=self.frequencies, layout=layout, out_layout=out_layout)

    @classmethod
    def from_sequential(cls, seq):
        """An nn.Sequential of [FrequencyEncoding,] Linear, (ReLU, Linear)* or Linear*, [Sigmoid | Tanh] -> TinyMLP holding clones of its
        parameters.  Identity modules are skipped; every Linear but the last is followed by a ReLU, or none is."""
        mods = [m for m in seq if not isinstance(m, torch.nn.Identity)]
        L = 0
        if mods and isinstance(mods[0], FrequencyEncoding):
            L, mods = mods[0].frequencies, mods[1:]
        outa = "none"
        if mods and isinstance(mods[-1], (torch.nn.Sigmoid, torch.nn.Tanh)):
            outa, mods = ("sigmoid" if isinstance(mods[-1], torch.nn.Sigmoid) else "tanh"), mods[:-1]
        linears = [m for m in mods if isinstance(m, torch.nn.Linear)]
        relus = [i for i, m in enumerate(mods) if isinstance(m, torch.nn.ReLU)]
        M = len(linears)
        if M == 0 or M > MAX_LAYERS or len(linears) + len(relus) != len(mods):
            raise ValueError(f"from_sequential reads [FrequencyEncoding,] 1..{MAX_LAYERS} Linear modules with ReLU between them and an "
                             f"optional Sigmoid or Tanh at the end; got {seq}")
        with_relu = [isinstance(m, torch.nn.Linear) for m in mods] == [True, False] * (M - 1) + [True]
        plain = len(relus) == 0
        if not (with_relu or plain):
            raise ValueError(f"from_sequential needs a ReLU behind every Linear but the last, or none at all; got {seq}")
        if any((l.bias is None) != (linears[0].bias is None) for l in linears):
            raise ValueError("from_sequential needs a bias on every Linear or on none")
        if linears[0].in_features % (1 + 2 * L):
            raise ValueError(f"from_sequential: the first Linear has {linears[0].in_features} inputs, no multiple of 1 + 2 x {L}")
        out = cls(linears[0].in_features // (1 + 2 * L), linears[-1].out_features, hidden=1, hidden_layers=0,
                  activation="relu" if with_relu and M > 1 else "none", output_activation=outa, frequencies=L)
        out.weights = torch.nn.ParameterList([torch.nn.Parameter(l.weight.detach().clone().float()) for l in linears])
        out.biases = None if linears[0].bias is None else torch.nn.ParameterList([torch.nn.Parameter(l.bias.detach().clone().float()) for l in linears])
        return out

    def to_sequential(self):
        """The stock modules with clones of the parameters: [FrequencyEncoding,] Linear, (ReLU, Linear)*, [Sigmoid | Tanh]"""
        mods = [FrequencyEncoding(self.frequencies)] if self.frequencies else []
        M = len(self.weights)
        for l, w in enumerate(self.weights):
            lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=self.biases is not None, device=w.device)
            with torch.no_grad():
                lin.weight.copy_(w)
                if self.biases is not None:
                    lin.bias.copy_(self.biases[l])
            mods.append(lin)
            if l < M - 1 and self.activation == "relu":
                mods.append(torch.nn.ReLU())
        if self.output_activation != "none":
            mods.append(torch.nn.Sigmoid() if self.output_activation == "sigmoid" else torch.nn.Tanh())
        return torch.nn.Sequential(*mods)


def decode_feature_map(feature_map, mlp_module):
    """feature_map (K, H, W) -> (C, H, W): the module applied to every pixel, reading the map as K planes in place and writing C planes.
    The gradient reaches the module's parameters and feature_map, and through the feature pass every Gaussian input."""
    if not torch.is_tensor(feature_map):
        raise TypeError("feature_map must be a tensor")
    if feature_map.dim() != 3:
        raise RuntimeError(f"feature_map must have dimensions (K, H, W); got {tuple(feature_map.shape)}")
    if not isinstance(mlp_module, TinyMLP):
        raise TypeError("mlp must be a TinyMLP")
    K, H, W = feature_map.shape
    if K != mlp_module.in_dim:
        raise RuntimeError(f"feature_map has {K} channels, the module reads {mlp_module.in_dim}")
    return mlp_module(feature_map.reshape(K, H * W), layout="planes").reshape(-1, H, W)
