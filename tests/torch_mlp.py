"""The references of the fused MLP (include/gsr_mlp.h), written from the header's rule and independently of the kernels.

    mlp_ref(x, Ws, bs, ...)            the rule in float64 torch operations (differentiable); absolute=True evaluates it on moduli
    backward_ref(x, Ws, bs, dy, ...)   the hand-written backward rule in float64 (test_mlp_cpu.py holds it against autograd)
    chain_fp32(W, a, b)                the float32 fmaf chain of one linear map, exactly, with the elements it cannot decide
    emulate(x, Ws, bs, dy, ...)        the whole float32 computation of the rule through chain_fp32 (output activation "none", L = 0)
    bars(...)                          the float64 check's error bars, from the computation re-run on moduli
    integer_case(...), general_case(...)   the fixtures of test_mlp_gpu.py; test_mlp_cpu.py asserts what they promise

Error bars.  u = 2^-24.  One chain of n fmas started at the bias has error at most gamma_n = n u / (1 - n u) times the chain on
moduli, |b| + sum |W||a|, and passes an error of its input on through |W|.  ReLU is 1-Lipschitz and an encoded sine or cosine carries
one rounding u, so to first order the error of z_l is at most
    E_l = gamma_{d_{l-1} + 1} (|b_l| + |W_l| |a_{l-1}|) + |W_l| E_{l-1},        E_0 = u on the encoded columns, 0 on x itself.
A row is *fragile* when some hidden |z_l| is at most its own E_l: there the float64 mask may differ from the float32 one, and such
rows are left out of the comparisons with float64 gradients.  With equal masks the same recursion runs down: dz_M carries its one
rounding and the move of act' under the error of z_M (|act''| <= 1 for the sigmoid and for tanh; nothing at all for "none"), and
    F_{l-1} = gamma_{d_l} |W_l|^T |dz_l| + |W_l|^T F_l   (zero where the mask is).
dW_l = sum dz_l a_{l-1} then has gamma_n sum |dz||a| of its own, n the additions into one element, plus sum F_l |a| + sum |dz| E(a);
db_l likewise; dx is F_0 carried through the encoding's chain rule, plus its one rounding."""
import math

import numpy as np
import torch

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- the rule in float64 -------------------------------------------------------------------------------------------------------------
def encode(x, L, absolute=False):
    """x (N, D) -> (N, D (1 + 2 L)): 2^j x is exact in float32 and in float64 alike; absolute: every block's modulus bound"""
    out = [x.abs() if absolute else x]
    for j in range(L):
        t = x * 2.0 ** j
        out += [torch.ones_like(x), torch.ones_like(x)] if absolute else [torch.sin(t), torch.cos(t)]
    return torch.cat(out, dim=1)


def out_act(z, name):
    return z if name == "none" else torch.sigmoid(z) if name == "sigmoid" else torch.tanh(z)


def mlp_ref(x, Ws, bs, activation="relu", output_activation="none", L=0, absolute=False, layers=False):
    """x (N, D) float64, Ws[l] (d_{l+1}, d_l), bs[l] or None -> y (N, d_M).  absolute: the same computation on moduli with the
    activations replaced by their Lipschitz bound 1 (the value is then a bound of |z_M|).  layers: also the list of every z_l."""
    a = encode(x, L, absolute)
    zs = []
    for l, W in enumerate(Ws):
        b = None if bs is None else bs[l]
        if absolute:
            z = a @ W.abs().T + (0 if b is None else b.abs())
        else:
            z = a @ W.T + (0 if b is None else b)
        zs.append(z)
        if l < len(Ws) - 1:
            a = z if (absolute or activation == "none") else torch.where(z <= 0, torch.zeros_like(z), z)
    y = zs[-1] if absolute else out_act(zs[-1], output_activation)
    return (y, zs) if layers else y


def backward_ref(x, Ws, bs, dy, activation="relu", output_activation="none", L=0, want_dx=True, want_dw=True, want_db=True):
    """The backward rule of the header, operation by operation in float64 -> (dx or None, [dW_l] or None, [db_l] or None)"""
    a = [encode(x, L)]
    zs = []
    M = len(Ws)
    for l, W in enumerate(Ws):
        z = a[-1] @ W.T + (0 if bs is None or bs[l] is None else bs[l])
        zs.append(z)
        if l < M - 1:
            a.append(z if activation == "none" else torch.where(z <= 0, torch.zeros_like(z), z))
    zM = zs[-1]
    if output_activation == "sigmoid":
        dz = dy * (torch.sigmoid(zM) * torch.sigmoid(-zM))
    elif output_activation == "tanh":
        dz = dy * (1 - torch.tanh(zM) ** 2)
    else:
        dz = dy
    dW, db = [None] * M, [None] * M
    for l in range(M - 1, -1, -1):
        dW[l] = dz.T @ a[l]
        db[l] = dz.sum(0)
        if l == 0 and not want_dx:
            break
        da = dz @ Ws[l]
        if l > 0:
            dz = da if activation == "none" else torch.where(zs[l - 1] > 0, da, torch.zeros_like(da))
    dx = None
    if want_dx:
        D = x.shape[1]
        dx = da[:, :D].clone()
        for j in range(L):
            t = x * 2.0 ** j
            gs, gc = da[:, D * (1 + 2 * j):D * (2 + 2 * j)], da[:, D * (2 + 2 * j):D * (3 + 2 * j)]
            dx = dx + 2.0 ** j * (torch.cos(t) * gs - torch.sin(t) * gc)
    return dx, (dW if want_dw else None), (db if want_db else None)


# ---- the float32 chain, exactly --------------------------------------------------------------------------------------------------------
def fma_fp32(w, a, acc):
    """float32(w a + acc) elementwise for float32 arrays -> (value float32, undecided bool).  The product of two float32 is exact in
    float64; the sum is rounded to float64 and then to float32, which differs from the single rounding of fmaf only where the float64
    sum lies exactly on a float32 rounding midpoint (its low 29 mantissa bits are 0x10000000) AND the float64 addition was inexact:
    the first rounding then moved the sum onto the tie, and the second breaks it without knowing from which side.  An exact float64
    sum on a midpoint is a true tie, which both roundings break to even alike; short products against a cancelling accumulator make
    those common (one in 10^6 steps), so the addition's exactness is read from its TwoSum error term.  Only the others are flagged."""
    p, c = w.astype(np.float64) * a.astype(np.float64), acc.astype(np.float64)
    s = p + c
    v = s - p
    err = (p - (s - v)) + (c - v)   # TwoSum: p + c = s + err exactly
    low = np.ascontiguousarray(s).view(np.uint64) & np.uint64(0x1FFFFFFF)
    with np.errstate(invalid="ignore"):
        return s.astype(np.float32), (low == np.uint64(0x10000000)) & (err != 0) & np.isfinite(s)


def chain_fp32(W, a, b=None):
    """z[n][o] = the chain acc = fmaf(W[o][k], a[n][k], acc), k ascending, started at b[o] (+0 without) -> (z (N, O) float32,
    undecided (N, O) bool: an element is undecided from the first flagged step on)"""
    W, a = np.asarray(W, np.float32), np.asarray(a, np.float32)
    N, O = a.shape[0], W.shape[0]
    acc = np.zeros((N, O), np.float32) if b is None else np.broadcast_to(np.asarray(b, np.float32), (N, O)).copy()
    und = np.zeros((N, O), bool)
    for k in range(W.shape[1]):
        acc, f = fma_fp32(W[None, :, k], a[:, k, None], acc)
        und |= f
    return acc, und


def emulate(x, Ws, bs, dy=None, activation="relu"):
    """The float32 computation of the rule for output activation "none" and no encoding -> dict(z (N, d_M), a [a_0 .. a_{M-1}],
    dz [dz_1 .. dz_M], dx, undecided (N,) bool: rows that hold an undecided element anywhere, forward or backward)"""
    a = [np.asarray(x, np.float32)]
    M = len(Ws)
    und = np.zeros((a[0].shape[0],), bool)
    z = None
    for l in range(M):
        z, f = chain_fp32(Ws[l], a[-1], None if bs is None else bs[l])
        und |= f.any(1)
        if l < M - 1:
            a.append(z if activation == "none" else np.where(z <= 0, np.float32(0), z))
    out = dict(z=z, a=a, undecided=und)
    if dy is not None:
        dz = [None] * M
        dz[M - 1] = np.asarray(dy, np.float32)
        for l in range(M - 1, -1, -1):
            da, f = chain_fp32(np.asarray(Ws[l], np.float32).T, dz[l])
            und |= f.any(1)
            if l > 0:
                dz[l - 1] = da if activation == "none" else np.where(a[l] > 0, da, np.float32(0))
        out.update(dz=dz, dx=da, undecided=und)
    return out


# ---- bars of the float64 check ---------------------------------------------------------------------------------------------------------
SECOND_ORDER = 1.001   # the bounds below are first order in u; the neglected products of two of them are below 1e-4 of them


def bars(x, Ws, bs, dy, activation="relu", output_activation="none", L=0, additions=None):
    """x, Ws, bs, dy float64 tensors -> dict(y, dx, dW [..], db [..], fragile (N,) bool): bounds of |float32 result - float64 result|
    by the module docstring's recursion, evaluated in float64.  additions: the terms added into one element of dW or db (default
    N + 256: a chain over the rows and a fold over at most 256 partials)."""
    M, N, D = len(Ws), x.shape[0], x.shape[1]
    n_add = N + 256 if additions is None else additions
    zero = torch.zeros((), dtype=torch.float64)
    bias = lambda l: zero if bs is None or bs[l] is None else bs[l].abs()
    # forward: E[l] bounds the error of z_{l+1}, Ea that of its input a_l
    a = [encode(x, L)]
    Ea = [torch.cat([torch.zeros_like(x)] + [U * torch.ones_like(x)] * (2 * L), dim=1)]   # the encoding's one rounding, |sin|, |cos| <= 1
    zs, E = [], []
    for l, W in enumerate(Ws):
        z = a[l] @ W.T + (0 if bs is None or bs[l] is None else bs[l])
        E.append(gamma(W.shape[1] + 1) * (a[l].abs() @ W.abs().T + bias(l)) + Ea[l] @ W.abs().T)
        zs.append(z)
        if l < M - 1:
            a.append(z if activation == "none" else torch.where(z <= 0, torch.zeros_like(z), z))
            Ea.append(E[l])   # ReLU is 1-Lipschitz
    fragile = torch.zeros(N, dtype=torch.bool)
    if activation == "relu":
        for l in range(M - 1):
            fragile |= (zs[l].abs() <= E[l]).any(1)
    y = out_act(zs[-1], output_activation)
    ybar = E[-1] + U * y.abs()   # |act'| <= 1, and the one rounding of y
    # backward: F bounds the error of dz_l given equal masks (rows where they may differ are fragile)
    if output_activation == "none":
        dz, F = dy, torch.zeros_like(dy)
    else:
        d1 = torch.sigmoid(zs[-1]) * torch.sigmoid(-zs[-1]) if output_activation == "sigmoid" else 1 - torch.tanh(zs[-1]) ** 2
        dz = dy * d1
        F = U * dz.abs() + dy.abs() * E[-1]   # its one rounding; act' moves by at most |act''| <= 1 times the error of z_M
    dWb, dbb = [None] * M, [None] * M
    for l in range(M - 1, -1, -1):
        dWb[l] = SECOND_ORDER * (gamma(n_add) * (dz.abs().T @ a[l].abs()) + F.T @ a[l].abs() + dz.abs().T @ Ea[l])
        dbb[l] = SECOND_ORDER * (gamma(n_add) * dz.abs().sum(0) + F.sum(0))
        F = gamma(Ws[l].shape[0]) * (dz.abs() @ Ws[l].abs()) + F @ Ws[l].abs()
        da = dz @ Ws[l]
        if l > 0:
            keep = torch.ones_like(da, dtype=torch.bool) if activation == "none" else zs[l - 1] > 0
            dz, F = torch.where(keep, da, torch.zeros_like(da)), torch.where(keep, F, torch.zeros_like(F))
    dx, Fx = da[:, :D].clone(), F[:, :D].clone()
    for j in range(L):
        t = x * 2.0 ** j
        s0, c0 = D * (1 + 2 * j), D * (2 + 2 * j)
        dx = dx + 2.0 ** j * (torch.cos(t) * da[:, s0:s0 + D] - torch.sin(t) * da[:, c0:c0 + D])
        Fx = Fx + 2.0 ** j * (F[:, s0:s0 + D] + F[:, c0:c0 + D])
    dxb = SECOND_ORDER * (Fx + (U * dx.abs() if L else 0))
    return dict(y=SECOND_ORDER * ybar, dx=dxb, dW=dWb, db=dbb, fragile=fragile)


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------
def integer_case(N, widths, seed, fan_in=6, bias=True, asymmetric=False):
    """Weights in {-1, 0, 1} with at most fan_in nonzeros per row and per column, inputs, biases and dy small integers: every partial
    sum of forward and backward stays far below 2^24 (test_mlp_cpu.py asserts it), so float32 is exact in any order.
    asymmetric: W_l[o][k] nonzero only for k = (o + l) mod d_{l-1}, with distinct values 1 + (o mod 3) -- a row / column swap, a wrong
    k half or a wrong layer-to-layer transpose moves a value to another place.  -> dict(x, Ws, bs, dy) of float32 numpy arrays"""
    rng = np.random.default_rng(seed)
    Ws, bs = [], []
    for l in range(1, len(widths)):
        din, dout = widths[l - 1], widths[l]
        W = np.zeros((dout, din), np.float32)
        if asymmetric:
            for o in range(dout):
                W[o, (o + l) % din] = 1 + o % 3
        else:
            for o in range(dout):
                ks = rng.choice(din, size=min(fan_in, din), replace=False)
                W[o, ks] = rng.choice([-1.0, 1.0], size=ks.size)
            for k in range(din):   # bounded fan-out as well: the backward chains run over the columns
                nz = np.flatnonzero(W[:, k])
                if nz.size > fan_in:
                    W[rng.choice(nz, size=nz.size - fan_in, replace=False), k] = 0
        Ws.append(W)
        bs.append(rng.integers(-2, 3, size=dout).astype(np.float32) if bias else None)
    x = rng.integers(-3, 4, size=(N, widths[0])).astype(np.float32)
    dy = rng.integers(-2, 3, size=(N, widths[-1])).astype(np.float32)
    return dict(x=x, Ws=Ws, bs=bs if bias else None, dy=dy)


def general_case(N, widths, seed, D=None):
    """weights ~ U(-1, 1) / sqrt(fan-in), biases ~ U(-1, 1) / sqrt(fan-in), inputs and dy ~ N(0, 1) -> dict(x (N, D or d_0), Ws, bs, dy)"""
    rng = np.random.default_rng(seed)
    Ws = [(rng.uniform(-1, 1, size=(widths[l], widths[l - 1])) / math.sqrt(widths[l - 1])).astype(np.float32) for l in range(1, len(widths))]
    bs = [(rng.uniform(-1, 1, size=widths[l]) / math.sqrt(widths[l - 1])).astype(np.float32) for l in range(1, len(widths))]
    x = rng.standard_normal((N, widths[0] if D is None else D)).astype(np.float32)
    dy = rng.standard_normal((N, widths[-1])).astype(np.float32)
    return dict(x=x, Ws=Ws, bs=bs, dy=dy)


def t64(case):
    """A fixture as float64 torch tensors -> (x, Ws, bs, dy)"""
    f = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    return f(case["x"]), [f(W) for W in case["Ws"]], (None if case["bs"] is None else [f(b) for b in case["bs"]]), f(case["dy"])


# the fixtures of test_mlp_gpu.py: name -> (constructor, arguments)
INTEGER_SHAPES = {
    # N, widths: input, hidden and output widths from {1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128}, M from {1, 2, 3, 5}
    "m1_tiny": (1, [3, 1]),
    "m1_odd": (31, [33, 65]),
    "m1_wide": (257, [128, 127]),
    "m2_a": (32, [1, 32, 2]),
    "m2_b": (33, [31, 63, 3]),
    "m2_c": (63, [64, 64, 64]),
    "m2_d": (1000, [65, 33, 31]),
    "m2_e": (64, [63, 3, 32]),
    "m3_a": (64, [2, 31, 65, 1]),
    "m3_b": (65, [32, 127, 128, 33]),
    "m3_c": (255, [63, 64, 32, 3]),
    "m3_d": (256, [127, 2, 128, 64]),
    "m3_e": (33, [32, 1, 3, 63]),
    "m5_a": (257, [3, 33, 64, 31, 63, 2]),
    "m5_b": (1000, [32, 64, 65, 64, 32, 3]),
    "m5_wide": (65, [128, 128, 128, 128, 128, 128]),
}
# N, widths, seed: the seeds are chosen so that at most 0.1 % of the outputs are undecided and 1 % of the rows fragile (test_mlp_cpu.py)
GENERAL_SHAPES = {
    "g_64x2": (1000, [32, 64, 64, 3], 2),
    "g_scaffold": (257, [35, 32, 70], 2),
    "g_odd": (333, [7, 33, 65, 31, 5], 3),
    "g_128": (130, [100, 128, 16], 1),   # two hidden layers of 128 make 8 % of the rows fragile by the rigorous E_l: the deep wide path is the integer cases'
}


def integer_fixture(name, asymmetric=False):
    N, widths = INTEGER_SHAPES[name]
    return integer_case(N, widths, seed=sum(map(ord, name)), asymmetric=asymmetric)


def general_fixture(name):
    N, widths, seed = GENERAL_SHAPES[name]
    return general_case(N, widths, seed=seed)


def encoded_fixture(L, D, seed=None):
    """D raw columns and L octaves -> 64 -> 64 -> 3 on 300 rows; x is scaled so that 2^(L-1) x stays within a few radians"""
    c = general_case(300, [D * (1 + 2 * L), 64, 64, 3], seed=ENCODED_SEEDS[(L, D)] if seed is None else seed, D=D)
    c["x"] = (c["x"] * (0.01 if L == 10 else 1.0)).astype(np.float32)
    return c


ENCODED_SEEDS = {(1, 5): 51, (10, 4): 51}   # (L, D) of test_mlp_gpu.test_frequency_encoding
