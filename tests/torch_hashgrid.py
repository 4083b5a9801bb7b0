"""The references of the hash-grid encoding (include/gsr_hashgrid.h), written from the header's rule and independently of the kernels.

    layout(cfg)                       the level table in numpy: scales (float32), resolutions, sizes, offsets, hashed flags
    level_terms(x, lay, l)            per row of one level: void flag, corner indices (N, 2^D), corner weights (float32), axis weights
    emulate_y(x, table, cfg)          the float32 fmaf chain of the header through torch_mlp.fma_fp32 -> (y, undecided)
    emulate_dtable(x, dy, cfg)        the integer rule in numpy int64: exact, for every input -> dtable float32 (info=True: also q, n_e)
    ref64(x, table, dy, cfg)          the rule in float64: y, analytic dx with the sum of its terms' moduli, dtable as a float64 sum
    hash_grid_torch(x, table, cfg)    the straightforward differentiable torch version (float64: the rule; float32: what one writes
                                      without this library -- gathers and, through autograd, an index_add_ backward)
    fragile_rows(x, cfg)              rows with a clamped coordinate times scale_l within 2^-18 of an integer at some level
    CONFIGS, integer_fixture(name), general_fixture(name)   the fixtures of test_hashgrid_gpu.py; test_hashgrid_cpu.py asserts what
                                      they promise

cfg = (D, L, F, log2_hashmap_size, base_resolution, per_level_scale)."""
import math

import numpy as np
import torch

import torch_mlp as tm

PRIMES = (1, 2654435761, 805459861, 3674653429)
LDS_BYTES = 128 * 1024   # GSR_HASHGRID_LDS_BYTES


def layout(cfg):
    D, L, F, T, base, pls = cfg
    scales, res, sizes, offs, hashed = [], [], [], [0], []
    for l in range(L):
        s = np.float32(np.exp2(np.float64(np.float32(l) * np.float32(np.log2(np.float64(np.float32(pls))))))) * np.float32(base) - np.float32(1)
        assert s.dtype == np.float32
        r = int(np.ceil(s)) + 1
        size = min((r ** D + 7) // 8 * 8, 1 << T)
        scales.append(s)
        res.append(r)
        sizes.append(size)
        hashed.append(r ** D > size)
        offs.append(offs[-1] + size)
    return dict(D=D, L=L, F=F, scales=np.array(scales, np.float32), res=res, sizes=sizes, offs=offs, hashed=hashed, total=offs[-1],
                lds=[(not h) and s * F * 8 <= LDS_BYTES for h, s in zip(hashed, sizes)])


def rows(x):
    """x (N, D) float32 -> (void (N,), clamped (N, D) bool, xc (N, D) float32)"""
    x = np.asarray(x, np.float32)
    void = ~np.isfinite(x).all(1)
    with np.errstate(invalid="ignore"):
        clamped = (x < 0) | (x > 1)
        xc = np.where(x < 0, np.float32(0), np.where(x > 1, np.float32(1), x)).astype(np.float32)
    xc[void] = 0   # never used: a void row takes no part
    return void, clamped, xc


def level_terms(x, lay, l):
    """-> void (N,), idx (N, 2^D) int64 within the level, w (N, 2^D) float32, u (N, 2^D, D) float32 axis weights, sign (2^D, D)"""
    D = lay["D"]
    void, clamped, xc = rows(x)
    p = xc.astype(np.float64) * np.float64(lay["scales"][l])
    p = p + 0.5
    cell = np.floor(p)
    frac = (p - cell).astype(np.float32)   # the difference is exact in double; the conversion rounds once
    c = cell.astype(np.uint32)
    K = 1 << D
    bits = np.array([[(k >> a) & 1 for a in range(D)] for k in range(K)], np.uint32)   # (K, D)
    g = c[:, None, :] + bits[None]                                                      # uint32, wrapping
    one_minus = (np.float32(1) - frac).astype(np.float32)
    u = np.where(bits[None].astype(bool), frac[:, None, :], one_minus[:, None, :]).astype(np.float32)
    w = u[:, :, 0].copy()
    for a in range(1, D):
        w = (w * u[:, :, a]).astype(np.float32)
    with np.errstate(over="ignore"):
        if lay["hashed"][l]:
            h = np.zeros(g.shape[:2], np.uint32)
            for a in range(D):
                h ^= g[:, :, a] * np.uint32(PRIMES[a])
        else:
            h = np.zeros(g.shape[:2], np.uint32)
            stride = np.uint32(1)
            for a in range(D):
                h += g[:, :, a] * stride
                stride = np.uint32((int(stride) * lay["res"][l]) & 0xFFFFFFFF)
    idx = (h.astype(np.int64) % lay["sizes"][l])
    sign = np.where(bits.astype(bool), 1.0, -1.0)
    return void, idx, w, u, sign


def emulate_y(x, table, cfg):
    """-> (y (N, L F) float32, undecided bool): the chain acc = fmaf(w_k, table[..][f], acc) over ascending corners from +0"""
    lay = layout(cfg)
    D, L, F = lay["D"], lay["L"], lay["F"]
    table = np.asarray(table, np.float32)
    N = len(x)
    y, und = np.zeros((N, L * F), np.float32), np.zeros((N, L * F), bool)
    for l in range(L):
        void, idx, w, _, _ = level_terms(x, lay, l)
        acc, flag = np.zeros((N, F), np.float32), np.zeros((N, F), bool)
        for k in range(1 << D):
            t = table[lay["offs"][l] + idx[:, k]]
            acc, f = tm.fma_fp32(w[:, k, None], t, acc)
            flag |= f
        acc[void], flag[void] = 0, False
        y[:, l * F:(l + 1) * F], und[:, l * F:(l + 1) * F] = acc, flag
    return y, und


def quantum(dy, N, D):
    """-> (kind, q): kind "nan" (m not finite), "zero" (m = 0) or "sum" with the rule's q"""
    bits = np.ascontiguousarray(dy, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    mbits = int(bits.max()) if bits.size else 0
    if mbits >= 0x7F800000:
        return "nan", None
    if mbits == 0:
        return "zero", None
    m = float(np.array([mbits], np.uint32).view(np.float32)[0])
    e = math.frexp(m)[1]   # m = f 2^e with f in [1/2, 1): e = ilogb(m) + 1
    B = (N * (1 << D) - 1).bit_length()
    return "sum", 62 - B - e


def emulate_dtable(x, dy, cfg, info=False):
    """The header's integer sum -> dtable (total, F) float32; info: (dtable, q, n_e (total,) terms per entry counting zero ones)"""
    lay = layout(cfg)
    D, L, F = lay["D"], lay["L"], lay["F"]
    dy = np.asarray(dy, np.float32)
    N = len(x)
    kind, q = quantum(dy, N, D) if N else ("zero", None)
    S = np.zeros(lay["total"] * F, np.int64)
    n_e = np.zeros(lay["total"], np.int64)
    if kind == "sum":
        for l in range(L):
            void, idx, w, _, _ = level_terms(x, lay, l)
            live = ~void
            prod = w[live].astype(np.float64)[:, :, None] * dy[live, None, l * F:(l + 1) * F].astype(np.float64)   # exact
            t = np.rint(np.ldexp(prod, q)).astype(np.int64)
            e = (lay["offs"][l] + idx[live])[:, :, None] * F + np.arange(F)[None, None]
            np.add.at(S, e.ravel(), t.ravel())
            np.add.at(n_e, (lay["offs"][l] + idx[live]).ravel(), 1)
        with np.errstate(over="ignore"):
            out = np.ldexp(S.astype(np.float64), -q).astype(np.float32)
    elif kind == "nan":
        out = np.full(lay["total"] * F, np.nan, np.float32)
    else:
        out = np.zeros(lay["total"] * F, np.float32)
    out = out.reshape(lay["total"], F)
    return (out, q, n_e) if info else out


def ref64(x, table, dy, cfg):
    """The rule in float64 -> dict(y (N, L F), dx (N, D), dx_abs (N, D): the sum of the moduli of dx's terms, dtable (total, F): the
    float64 sum of w dy, dtable_abs).  frac, the axis weights and the corner weight w of y and dtable are the rule's float32 values;
    everything after them is double (dx takes its products of axis weights in double, as the header says)."""
    lay = layout(cfg)
    D, L, F = lay["D"], lay["L"], lay["F"]
    table64, dy64 = np.asarray(table, np.float64), None if dy is None else np.asarray(dy, np.float64)
    N = len(x)
    void, clamped, _ = rows(x)
    y = np.zeros((N, L * F))
    dx, dx_abs = np.zeros((N, D)), np.zeros((N, D))
    dt, dt_abs = np.zeros((lay["total"], F)), np.zeros((lay["total"], F))
    for l in range(L):
        _, idx, w, u, sign = level_terms(x, lay, l)
        w = w.astype(np.float64)
        t = table64[lay["offs"][l] + idx]                       # (N, K, F)
        yl = (w[:, :, None] * t).sum(1)
        yl[void] = 0
        y[:, l * F:(l + 1) * F] = yl
        if dy64 is None:
            continue
        g = dy64[:, l * F:(l + 1) * F]
        s = (g[:, None, :] * t).sum(2)                          # (N, K)
        s_abs = (np.abs(g)[:, None, :] * np.abs(t)).sum(2)
        u64 = u.astype(np.float64)
        for a in range(D):
            others = np.ones(u64.shape[:2])
            for b in range(D):
                if b != a:
                    others = others * u64[:, :, b]
            dx[:, a] += (np.float64(lay["scales"][l]) * sign[None, :, a] * others * s).sum(1)
            dx_abs[:, a] += (np.float64(lay["scales"][l]) * others * s_abs).sum(1)
        live = ~void
        term = w[live][:, :, None] * g[live, None, :]
        e = lay["offs"][l] + idx[live]
        np.add.at(dt, e.ravel(), term.reshape(-1, F))
        np.add.at(dt_abs, e.ravel(), np.abs(term).reshape(-1, F))
    dx[void], dx_abs[void] = 0, 0
    dx[clamped & ~void[:, None]] = 0
    return dict(y=y, dx=dx, dx_abs=dx_abs, dtable=dt, dtable_abs=dt_abs)


def fragile_rows(x, cfg):
    """Rows where a clamped coordinate times scale_l lies within 2^-18 of an integer at some level (void rows are never fragile)"""
    lay = layout(cfg)
    void, _, xc = rows(x)
    out = np.zeros(len(xc), bool)
    for l in range(lay["L"]):
        v = xc.astype(np.float64) * np.float64(lay["scales"][l])
        out |= (np.abs(v - np.rint(v)) < 2.0 ** -18).any(1)
    return out & ~void


# ---- the straightforward torch version -------------------------------------------------------------------------------------------------
def hash_grid_torch(x, table, cfg):
    """Differentiable w.r.t. x and table.  table float64: the header's rule (x holds float32 values; frac, the axis weights and the
    corner weights take the rule's float32 values, and the derivatives run in double: x.grad is the header's dx, table.grad the float64
    sum of w dy).  table float32: every operation in float32, as one writes it without the library."""
    D, L, F, T, base, pls = cfg
    lay = layout(cfg)
    dt = table.dtype
    dev = x.device
    void = ~torch.isfinite(x).all(1)
    xc = torch.where(void[:, None], torch.zeros_like(x), x).clamp(0, 1).to(dt)
    K = 1 << D
    bits = torch.tensor([[(k >> a) & 1 for a in range(D)] for k in range(K)], device=dev)   # (K, D)
    primes = torch.tensor(PRIMES[:D], dtype=torch.int64, device=dev)
    out = []
    for l in range(L):
        p = xc * float(lay["scales"][l]) + 0.5
        cell = torch.floor(p).detach()
        frac = p - cell
        if dt == torch.float64:   # the rule's float32 values of frac and 1 - frac, with the derivatives +1 and -1 kept in double
            f32 = frac.detach().float()
            u1, u0 = frac + (f32.double() - frac).detach(), -frac + ((1 - f32).double() + frac).detach()
        else:
            u1, u0 = frac, 1 - frac
        g = cell.long()[:, None, :] + bits[None]                                            # (N, K, D)
        if lay["hashed"][l]:
            h = torch.zeros(g.shape[:2], dtype=torch.int64, device=dev)
            for a in range(D):
                h = h ^ ((g[:, :, a] * primes[a]) & 0xFFFFFFFF)
        else:
            h = torch.zeros(g.shape[:2], dtype=torch.int64, device=dev)
            for a in range(D):
                h = h + g[:, :, a] * ((lay["res"][l] ** a) & 0xFFFFFFFF)
            h = h & 0xFFFFFFFF
        idx = h % lay["sizes"][l] + lay["offs"][l]
        u = torch.where(bits[None].bool(), u1[:, None, :], u0[:, None, :])                  # (N, K, D)
        w = u[:, :, 0]
        for a in range(1, D):
            w = w * u[:, :, a]
        if dt == torch.float64:   # the rule's corner weight, a float32 product, as the value; its derivative from the double products
            u32 = torch.where(bits[None].bool(), f32[:, None, :], (1 - f32)[:, None, :])
            w32 = u32[:, :, 0]
            for a in range(1, D):
                w32 = w32 * u32[:, :, a]
            w = w + (w32.double() - w).detach()
        t = table.index_select(0, idx.reshape(-1)).view(idx.shape[0], K, F)   # its backward is an index_add_ into the table's gradient
        yl = (w[:, :, None] * t).sum(1)
        out.append(torch.where(void[:, None], torch.zeros_like(yl), yl))
    return torch.cat(out, 1)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------
CONFIGS = {
    # everything in one: resolutions 2, 4, 8, 16, 32 -> an 8-entry level (a thousand terms per entry at N = 1000), LDS levels up to
    # 512 entries, res 16 dense with res^3 == 2^12 exactly and, at F = 8, beyond the LDS budget (direct), then the hashed level
    "all3": (3, 5, 8, 12, 2, 2.0),
    "seam3": (3, 3, 2, 12, 8, 2.0),        # res 8 (LDS), 16 (4096 == 2^12 exactly: dense, LDS at F = 2), 32 (hashed, direct)
    "budget2": (2, 3, 2, 14, 64, 1.5),     # res 64 (4096 entries, LDS), 96 (9216 entries, dense but beyond the budget), 144 (hashed)
    "tiny2": (2, 3, 4, 4, 2, 2.0),         # 2^4: res 2 (8 entries), res 4 (16 == 2^4 exactly, dense), res 8 (hashed into 16 entries)
    "int2": (2, 3, 2, 10, 4, 2.0),         # dense only with growth 2: 16, 64, 256 entries
    "dense2": (2, 3, 1, 12, 4, 1.5),       # dense only, F = 1, sizes that are no power of two (the mod, not the mask)
    "hashed2": (2, 3, 8, 4, 16, 2.0),      # hashed only, F = 8, hundreds of terms per entry
    "dense3": (3, 1, 4, 12, 5, 1.0),       # one dense level, 125 -> 128 entries
    "hashed3": (3, 3, 1, 10, 16, 1.5),     # hashed only
    "dense4": (4, 3, 2, 12, 2, 1.5),       # D = 4 dense: res 2, 3, 5
    "seam4": (4, 3, 1, 10, 3, 2.0),        # D = 4: res 3 (81 -> 88 entries, dense), 6 and 12 (hashed)
    "hashed4": (4, 8, 8, 10, 8, 1.3),      # D = 4, F = 8, L = 8: hashed only
}
# growth 2 (or 1) and an integer base: scale_l + 1 is an integer, so x on multiples of 1/4 has frac in {0, 1/4, 1/2, 3/4} at every level
INTEGER_CONFIGS = ("all3", "seam3", "tiny2", "int2", "hashed2", "dense3", "seam4")


def integer_fixture(name, N=257, seed=0):
    """x on multiples of 2^-2, so that x scale_l = x (scale_l + 1) - x is a multiple of 1/4 and every frac lies in {0, 1/4, 1/2, 3/4}:
    rows on cell faces, in cell centres, x = 0 and x = 1 (the top cell's +1 corner).  Small-integer table and dy.  Every weight is a
    multiple of 4^-D, so y, dtable and dx are exact in float32, in int64 and in float64 alike (test_hashgrid_cpu.py asserts it)."""
    cfg = CONFIGS[name]
    assert name in INTEGER_CONFIGS
    D, L, F = cfg[:3]
    lay = layout(cfg)
    rng = np.random.default_rng(1000 + seed)
    x = (rng.integers(0, 5, (N, D)) / 4.0).astype(np.float32)
    x[0] = 0.0
    x[1 % N] = 1.0
    table = rng.integers(-4, 5, (lay["total"], F)).astype(np.float32)
    dy = rng.integers(-3, 4, (N, L * F)).astype(np.float32)
    return dict(cfg=cfg, x=x, table=table, dy=dy)


def general_fixture(name, N=1000, seed=0, outside=True):
    """Random x in [0, 1) (with `outside`, three rows with a coordinate outside it and three void rows), normal table and dy"""
    cfg = CONFIGS[name]
    D, L, F = cfg[:3]
    lay = layout(cfg)
    rng = np.random.default_rng(2000 + seed + sum(map(ord, name)))
    x = rng.random((N, D), np.float32)
    if outside and N >= 16:
        x[3, 0], x[5, D - 1], x[7, 1] = -0.25, 1.5, -3.0
        x[9, 0], x[11, 1], x[13, D - 1] = np.nan, np.inf, -np.inf
    table = rng.standard_normal((lay["total"], F)).astype(np.float32)
    dy = rng.standard_normal((N, L * F)).astype(np.float32)
    return dict(cfg=cfg, x=x, table=table, dy=dy)
