"""The references of the HexPlane / K-Planes plane-grid encoding (include/gsr_hexplane.h), written from the header's rule and
independently of the kernels.

    Cfg(D, C, res, concat)            res[l][a]; planes(cfg), shapes(cfg), offsets(cfg), total(cfg), lds(cfg)
    unpack(table, cfg)                the flat table -> grids[l][k] of (1, C, res_b, res_a) tensors (views)
    hex_plane_torch(x, table, cfg)    (a) the straightforward differentiable torch version: F.grid_sample(bilinear, align_corners=True,
                                      padding_mode="border") per plane, product over the planes; float64 or float32 by the table's dtype
    ref64(x, table, dy, cfg)          (b) the header's rule in float64: y, analytic dx with the sum of its terms' moduli, dtable as a
                                      float64 sum.  frac32=True: frac and the corner weights take the rule's float32 values (what the
                                      kernels are held to); frac32=False: they stay double, which is what grid_sample computes in float64
    emulate_y(x, table, cfg)          (c) the float32 rule through torch_mlp.fma_fp32 -> (y, undecided, p): an element is undecided
                                      when a step of one of its chains fell on a double-rounding tie; p, the per-plane values the
                                      table gradient is formed from, has those steps resolved exactly from the TwoSum error term
    emulate_dtable(x, table, dy, cfg) (c) the integer rule in numpy int64: exact, for every input -> dtable float32 (info=True: also
                                      q per plane, n_e per node, the largest |t| 2^-(62-B))
    regularizer_torch(table, cfg, ..) (d) the regulariser in torch, float64 for a float64 table
    CONFIGS, integer_fixture(name), general_fixture(name), one_cell_fixture(name)   the fixtures of test_hexplane_gpu.py;
                                      test_hexplane_cpu.py asserts what they promise"""
import itertools
import math
from collections import namedtuple

import numpy as np
import torch

import torch_mlp as tm

Cfg = namedtuple("Cfg", "D C res concat")
LDS_BYTES = 128 * 1024   # GSR_HEXPLANE_LDS_BYTES


def planes(cfg):
    return list(itertools.combinations(range(cfg.D), 2))


def shapes(cfg):
    """[(l, k, a, b, res_b, res_a)] in the table's order"""
    return [(l, k, a, b, cfg.res[l][b], cfg.res[l][a]) for l in range(len(cfg.res)) for k, (a, b) in enumerate(planes(cfg))]


def offsets(cfg):
    off = [0]
    for _, _, _, _, rb, ra in shapes(cfg):
        off.append(off[-1] + rb * ra * cfg.C)
    return off


def total(cfg):
    return offsets(cfg)[-1]


def lds(cfg):
    """[l][k] True where the table backward takes the LDS path"""
    P = len(planes(cfg))
    flat = [rb * ra * 4 * 8 <= LDS_BYTES for _, _, _, _, rb, ra in shapes(cfg)]
    return [flat[l * P:(l + 1) * P] for l in range(len(cfg.res))]


def out_dim(cfg):
    return len(cfg.res) * cfg.C if cfg.concat else cfg.C


def unpack(table, cfg):
    grids, off = [[] for _ in cfg.res], offsets(cfg)
    for j, (l, _, _, _, rb, ra) in enumerate(shapes(cfg)):
        grids[l].append(table[off[j]:off[j + 1]].view(rb, ra, cfg.C).permute(2, 0, 1)[None])
    return grids


# ---- (a) the straightforward torch version ----------------------------------------------------------------------------------------------
def hex_plane_torch(x, table, cfg):
    """Differentiable w.r.t. x and table; x is converted to the table's dtype.  Void rows give zeros and take no part."""
    void = ~torch.isfinite(x).all(1)
    xs = torch.where(void[:, None], torch.zeros_like(x), x).to(table.dtype)
    out = []
    for level in unpack(table, cfg):
        z = None
        for (a, b), g in zip(planes(cfg), level):
            grid = torch.stack([xs[:, a], xs[:, b]], 1)[None, :, None, :]   # (1, N, 1, 2): the first coordinate indexes res_a (the width)
            p = torch.nn.functional.grid_sample(g, grid, mode="bilinear", padding_mode="border", align_corners=True)[0, :, :, 0].t()
            z = p if z is None else z * p
        out.append(torch.where(void[:, None], torch.zeros_like(z), z))
    if cfg.concat:
        return torch.cat(out, 1)
    y = torch.zeros_like(out[0])
    for z in out:
        y = y + z
    return y


# ---- the rule's per-row pieces ------------------------------------------------------------------------------------------------------------
def rows(x):
    """x (N, D) float32 -> (void (N,), clamped (N, D) bool)"""
    x = np.asarray(x, np.float32)
    void = ~np.isfinite(x).all(1)
    with np.errstate(invalid="ignore"):
        clamped = (x <= -1) | (x >= 1)
    return void, clamped


def level_terms(x, cfg, l):
    """-> i0 (N, D) int64, frac (N, D) float64 (the unrounded difference; its float32 rounding is the rule's frac).  Void rows get 0."""
    x = np.asarray(x, np.float32)
    void, _ = rows(x)
    u = np.where(void[:, None], np.float32(0), x).astype(np.float64)
    top = np.array(cfg.res[l], np.float64) - 1.0
    s = ((u + 1.0) * 0.5) * top
    s = np.minimum(np.maximum(s, 0.0), top)
    i0 = np.minimum(np.floor(s), top - 1.0)
    return i0.astype(np.int64), s - i0


def corner_nodes(i0, a, b, ra):
    """-> (N, 4) node indices ib * res_a + ia in the corner order (b0,a0), (b0,a1), (b1,a0), (b1,a1)"""
    n = i0[:, b] * ra + i0[:, a]
    return np.stack([n, n + 1, n + ra, n + ra + 1], 1)


def weights32(frac, a, b):
    """The rule's float32 corner weights w_b * w_a -> (N, 4) float32"""
    f = frac.astype(np.float32)
    fa, fb = f[:, a], f[:, b]
    a0, b0 = (np.float32(1) - fa).astype(np.float32), (np.float32(1) - fb).astype(np.float32)
    return np.stack([b0 * a0, b0 * fa, fb * a0, fb * fa], 1).astype(np.float32)


def level_dy(dy, cfg, l):
    return dy[:, l * cfg.C:(l + 1) * cfg.C] if cfg.concat else dy


# ---- (c) the exact emulation --------------------------------------------------------------------------------------------------------------
def fma_exact(w, a, acc):
    """fmaf(w, a, acc) elementwise for float32 arrays -> (value float32, flagged bool).  torch_mlp.fma_fp32 rounds the exact product
    plus acc to float64 and then to float32, and flags the steps where the float64 sum was inexact and fell on a float32 midpoint;
    there the exact sum lies on the side the TwoSum error term points to, so the single rounding of fmaf is known after all."""
    v, flag = tm.fma_fp32(w, a, acc)
    if flag.any():
        p, c = w.astype(np.float64) * a.astype(np.float64), acc.astype(np.float64)
        p, c = np.broadcast_arrays(p, c)
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)
        down, up = np.nextafter(s.astype(np.float32), np.float32(-np.inf)), np.nextafter(s.astype(np.float32), np.float32(np.inf))
        lo = np.where(s.astype(np.float32).astype(np.float64) > s, down, s.astype(np.float32))   # the float32 neighbours of the midpoint s
        hi = np.where(s.astype(np.float32).astype(np.float64) > s, s.astype(np.float32), up)
        v = np.where(flag, np.where(err > 0, hi, lo), v).astype(np.float32)
    return v, flag


def emulate_y(x, table, cfg):
    """-> (y (N, out_dim) float32, undecided bool of y's shape, p[l][k] (N, C) float32 exact)"""
    table = np.asarray(table, np.float32)
    N, C, L = len(x), cfg.C, len(cfg.res)
    void, _ = rows(x)
    off = offsets(cfg)
    P = len(planes(cfg))
    zs, unds, ps = [], [], []
    for l in range(L):
        i0, frac = level_terms(x, cfg, l)
        z, und, pl = None, np.zeros((N, C), bool), []
        for k, (a, b) in enumerate(planes(cfg)):
            ra = cfg.res[l][a]
            plane = table[off[l * P + k]:off[l * P + k + 1]].reshape(-1, C)
            nodes, w = corner_nodes(i0, a, b, ra), weights32(frac, a, b)
            acc = np.zeros((N, C), np.float32)
            for n in range(4):
                acc, f = fma_exact(w[:, n, None], plane[nodes[:, n]], acc)
                und |= f
            pl.append(acc)
            z = acc if z is None else (z * acc).astype(np.float32)
        z = z.copy()
        z[void], und[void] = 0, False
        zs.append(z)
        unds.append(und)
        ps.append(pl)
    if cfg.concat:
        return np.concatenate(zs, 1), np.concatenate(unds, 1), ps
    y, und = np.zeros((N, C), np.float32), np.zeros((N, C), bool)
    for z, u in zip(zs, unds):
        y, und = (y + z).astype(np.float32), und | u
    return y, und, ps


def _maxbits(a):
    bits = np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return int(bits.max()) if bits.size else 0


def _from_bits(b):
    return float(np.array([b], np.uint32).view(np.float32)[0])


def quanta(table, dy, cfg, N):
    """-> ("nan", None) or ("sum", q[l][k]) with q None for a plane that is +0 throughout; B = the smallest integer with 2^B >= 4 N"""
    off, P = offsets(cfg), len(planes(cfg))
    table = np.asarray(table, np.float32)
    mb = _maxbits(dy)
    Mb = [_maxbits(table[off[j]:off[j + 1]]) for j in range(len(off) - 1)]
    if mb >= 0x7F800000 or any(v >= 0x7F800000 for v in Mb):
        return "nan", None
    B = (4 * N - 1).bit_length()
    q = []
    for l in range(len(cfg.res)):
        q.append([])
        for k in range(P):
            bnd = _from_bits(mb)
            for j in range(P):
                if j != k:
                    bnd = bnd * _from_bits(Mb[l * P + j])
            if bnd == 0:
                q[-1].append(None)
                continue
            e = math.frexp(bnd)[1] + 1   # bnd = f 2^e' with f in [1/2, 1): ilogb = e' - 1
            q[-1].append(62 - B - e)
    return "sum", q


def emulate_dtable(x, table, dy, cfg, info=False):
    """The header's integer sum -> dtable (total,) float32; info: (dtable, q[l][k], n_e (total / C,) terms per node counting zero
    ones, the largest |t| over 2^(62 - B))"""
    table, dy = np.asarray(table, np.float32), np.asarray(dy, np.float32)
    N, C, P = len(x), cfg.C, len(planes(cfg))
    off = offsets(cfg)
    S = np.zeros(off[-1], np.int64)
    n_e = np.zeros(off[-1] // C, np.int64)
    kind, q = quanta(table, dy, cfg, N) if N else ("sum", [[None] * P for _ in cfg.res])
    worst = 0.0
    out = np.zeros(off[-1], np.float32)
    if kind == "nan":
        out[:] = np.nan
    else:
        B = (4 * N - 1).bit_length() if N else 0
        void, _ = rows(x)
        live = ~void
        _, _, ps = emulate_y(x, table, cfg)
        for l in range(len(cfg.res)):
            i0, frac = level_terms(x, cfg, l)
            g0 = level_dy(dy, cfg, l).astype(np.float64)
            for k, (a, b) in enumerate(planes(cfg)):
                j = l * P + k
                nodes, w = corner_nodes(i0, a, b, cfg.res[l][a])[live], weights32(frac, a, b)[live].astype(np.float64)
                np.add.at(n_e, off[j] // C + nodes.ravel(), 1)
                if q[l][k] is None:
                    continue
                g = g0.copy()
                for jj in range(P):
                    if jj != k:
                        g = g * ps[l][jj].astype(np.float64)
                g = g[live]
                for n in range(4):
                    prod = w[:, n, None] * g
                    t = np.rint(np.ldexp(prod, q[l][k]))
                    worst = max(worst, float(np.abs(t).max()) / 2.0 ** (62 - B)) if t.size else worst
                    e = off[j] + nodes[:, n, None] * C + np.arange(C)[None]
                    np.add.at(S, e.ravel(), t.astype(np.int64).ravel())
                with np.errstate(over="ignore"):
                    out[off[j]:off[j + 1]] = np.ldexp(S[off[j]:off[j + 1]].astype(np.float64), -q[l][k]).astype(np.float32)
    return (out, q, n_e, worst) if info else out


# ---- (b) the rule in float64 ----------------------------------------------------------------------------------------------------------------
def ref64(x, table, dy, cfg, frac32=True):
    """-> dict(y (N, out_dim), dx (N, D), dx_abs: the sum of the moduli of dx's terms, dtable (total,): the float64 sum of w g,
    dtable_abs).  dy None: y alone."""
    table64 = np.asarray(table, np.float64)
    N, C, D, L, P = len(x), cfg.C, cfg.D, len(cfg.res), len(planes(cfg))
    off = offsets(cfg)
    void, clamped = rows(x)
    live = ~void
    zs = []
    dx, dx_abs = np.zeros((N, D)), np.zeros((N, D))
    dt, dt_abs = np.zeros(off[-1]), np.zeros(off[-1])
    dy64 = None if dy is None else np.asarray(dy, np.float64)
    # the rule forms g_k from the float32 p_j: with frac32 the gradients take them from the exact emulation
    ps = emulate_y(x, table, cfg)[2] if frac32 and dy is not None else None
    for l in range(L):
        i0, frac = level_terms(x, cfg, l)
        f = frac.astype(np.float32).astype(np.float64) if frac32 else frac
        f0 = (np.float32(1) - frac.astype(np.float32)).astype(np.float64) if frac32 else 1.0 - frac
        p, da, db, aa, ws, nds = [], [], [], [], [], []
        for k, (a, b) in enumerate(planes(cfg)):
            ra = cfg.res[l][a]
            plane = table64[off[l * P + k]:off[l * P + k + 1]].reshape(-1, C)
            nodes = corner_nodes(i0, a, b, ra)
            v = [plane[nodes[:, n]] for n in range(4)]
            if frac32:
                w = weights32(frac, a, b).astype(np.float64)
            else:
                w = np.stack([f0[:, b] * f0[:, a], f0[:, b] * f[:, a], f[:, b] * f0[:, a], f[:, b] * f[:, a]], 1)
            p.append(sum(w[:, n, None] * v[n] for n in range(4)))
            da.append(f0[:, b, None] * (v[1] - v[0]) + f[:, b, None] * (v[3] - v[2]))
            db.append(f0[:, a, None] * (v[2] - v[0]) + f[:, a, None] * (v[3] - v[1]))
            aa.append((f0[:, b, None] * (np.abs(v[1]) + np.abs(v[0])) + f[:, b, None] * (np.abs(v[3]) + np.abs(v[2])),     # the moduli of da's terms
                       f0[:, a, None] * (np.abs(v[2]) + np.abs(v[0])) + f[:, a, None] * (np.abs(v[3]) + np.abs(v[1]))))    # and of db's
            ws.append(w)
            nds.append(nodes)
        z = np.prod(np.stack(p), 0)
        z[void] = 0
        zs.append(z)
        if dy64 is None:
            continue
        g0 = level_dy(dy64, cfg, l)
        pg = p if ps is None else [v.astype(np.float64) for v in ps[l]]
        for k, (a, b) in enumerate(planes(cfg)):
            g = g0.copy()
            for j in range(P):
                if j != k:
                    g = g * pg[j]
            ha, hb = (cfg.res[l][a] - 1) * 0.5, (cfg.res[l][b] - 1) * 0.5
            dx[:, a] += (g * ha * da[k]).sum(1)
            dx[:, b] += (g * hb * db[k]).sum(1)
            dx_abs[:, a] += (np.abs(g) * ha * aa[k][0]).sum(1)
            dx_abs[:, b] += (np.abs(g) * hb * aa[k][1]).sum(1)
            j = l * P + k
            for n in range(4):
                term = ws[k][live][:, n, None] * g[live]
                e = off[j] + nds[k][live][:, n, None] * C + np.arange(C)[None]
                np.add.at(dt, e.ravel(), term.ravel())
                np.add.at(dt_abs, e.ravel(), np.abs(term).ravel())
    y = np.concatenate(zs, 1) if cfg.concat else sum(zs)
    dx[void], dx_abs[void] = 0, 0
    dx[clamped & live[:, None]] = 0
    return dict(y=y, dx=dx, dx_abs=dx_abs, dtable=dt, dtable_abs=dt_abs)


# ---- (d) the regulariser ------------------------------------------------------------------------------------------------------------------
def regularizer_torch(table, cfg, tv_space=0.0, tv_time=0.0, smooth_space=0.0, smooth_time=0.0, l1_time=0.0):
    """K-Planes' plane regularisers on the unpacked (1, C, res_b, res_a) planes, differentiable in table"""
    total_ = table.new_zeros(())
    for level in unpack(table, cfg):
        for (a, b), g in zip(planes(cfg), level):
            _, C, h, w = g.shape
            tv = 2 * ((g[:, :, 1:, :] - g[:, :, :-1, :]).square().sum() / ((h - 1) * w * C) + (g[:, :, :, 1:] - g[:, :, :, :-1]).square().sum() / (h * (w - 1) * C))
            if h >= 3:
                first = g[:, :, 1:, :] - g[:, :, :-1, :]
                smooth = (first[:, :, 1:, :] - first[:, :, :-1, :]).square().mean()
            else:
                smooth = table.new_zeros(())
            if b == 3:
                total_ = total_ + tv_time * tv + smooth_time * smooth + l1_time * (1 - g).abs().mean()
            else:
                total_ = total_ + tv_space * tv + smooth_space * smooth
    return total_


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------------
def _multires(base, factors):
    return tuple(tuple(r * m if a < 3 else r for a, r in enumerate(base)) for m in factors)


CONFIGS = {
    "r2_d4": Cfg(4, 4, ((2, 2, 2, 2),), True),                                   # the smallest plane there is: i0 = 0 = res - 2 always
    "odd_d4": Cfg(4, 12, ((3, 5, 4, 2),), True),                                 # all resolutions different: a swapped axis shows
    "multi_d4": Cfg(4, 32, _multires((8, 8, 8, 4), (1, 2)), False),             # two levels summed, the time axis kept
    "multi_d3": Cfg(3, 64, _multires((8, 8, 8), (1, 2)) + ((3, 5, 4),), True),  # three levels, a full wave of channels
    "seam_d4": Cfg(4, 4, ((64, 64, 2, 2), (65, 64, 2, 2)), False),              # 64 x 64 nodes: the LDS budget exactly; 65 x 64: beyond
    "direct_d3": Cfg(3, 12, ((65, 64, 2), (3, 5, 4)), True),                     # a direct plane at C = 12 (lanes that straddle rows)
    "direct_d4": Cfg(4, 32, ((65, 64, 3, 2), (4, 4, 4, 3)), True),               # a direct plane at C = 32 beside time planes
}
# per axis res - 1 = R 2^l with R a power of two: u = -1 + j / R puts s on nodes and half nodes at level 0 and on nodes above it
INTEGER_CONFIGS = {
    "int_d4": Cfg(4, 4, ((3, 5, 2, 2), (5, 9, 3, 3)), True),
    "int_d3": Cfg(3, 12, ((2, 3, 5), (3, 5, 9), (5, 9, 17)), False),
    "int_seam": Cfg(3, 4, ((65, 65, 2),), True),                                 # 65 x 65 nodes: the direct path
}


def integer_fixture(name, N=257, seed=0):
    """u on nodes and half nodes of level 0 (nodes of the finer levels), u = -1 and u = +1 among them; plane values in {-1, +1},
    small-integer dy.  Every weight is a multiple of 1/4 and every product stays below 2^24, so y, dtable and dx are exact in
    float32, in int64 and in float64 alike (test_hexplane_cpu.py asserts it)."""
    cfg = INTEGER_CONFIGS[name]
    rng = np.random.default_rng(3000 + seed)
    R = np.array(cfg.res[0]) - 1
    x = (-1.0 + rng.integers(0, 2 * R + 1, (N, cfg.D)) / R).astype(np.float32)
    x[0], x[1 % N] = -1.0, 1.0
    table = rng.choice(np.array([-1.0, 1.0], np.float32), total(cfg))
    dy = rng.integers(-3, 4, (N, out_dim(cfg))).astype(np.float32)
    return dict(cfg=cfg, x=x, table=table, dy=dy)


def general_fixture(name, N=1000, seed=0, outside=True):
    """Random x in (-1, 1) (with `outside`, rows with a coordinate exactly -1, exactly +1 and beyond, and three void rows), normal
    table and dy"""
    cfg = CONFIGS[name]
    rng = np.random.default_rng(4000 + seed + sum(map(ord, name)))
    x = (rng.random((N, cfg.D), np.float32) * 2 - 1).astype(np.float32)
    if outside and N >= 16:
        x[2, 0], x[3, 1], x[4, cfg.D - 1] = -1.0, 1.0, 1.0
        x[5, 0], x[6, cfg.D - 1], x[7, 1] = -1.25, 1.5, -3.0
        x[9, 0], x[11, 1], x[13, cfg.D - 1] = np.nan, np.inf, -np.inf
    table = rng.standard_normal(total(cfg)).astype(np.float32)
    dy = rng.standard_normal((N, out_dim(cfg))).astype(np.float32)
    return dict(cfg=cfg, x=x, table=table, dy=dy)


def one_cell_fixture(name, N=1000, seed=0):
    """Every row inside one cell of every plane of level 0: a thousand terms per corner node"""
    c = general_fixture(name, N, seed, outside=False)
    rng = np.random.default_rng(5000 + seed)
    top = np.array(c["cfg"].res[0], np.float64) - 1
    cell = np.minimum(np.floor(0.6 * top), top - 1)
    s = cell + 0.05 + 0.9 * rng.random((N, c["cfg"].D))
    c["x"] = (s / top * 2 - 1).astype(np.float32)
    return c
