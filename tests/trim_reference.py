"""numpy restatement of the trim word's producer, csrc/gsr_rect_trim.h gsr_rect_trim(), and of what it is measured against.

rect_trim() repeats gsr_rect_trim() operation for operation in scalar np.float32: the same order, no fused multiply-add (the
geometry kernel is compiled without contraction).  The one difference: the kernel's reciprocal, square root and logarithm
(v_rcp_f32, v_sqrt_f32, v_log_f32) are good to 1 ulp, the ones here are correctly rounded.  So a word from here is the word of the
ALGEBRA -- what tests/test_trim_needles_cpu.py needs to change the bound and check it again without a GPU; the device's words are
judged by tests/test_trim_needles_gpu.py.  A change of gsr_rect_trim() has to be repeated in rect_trim().

Also here:
  * conic_radius_rect(): the reference's conic, radius and getRect for a given cov2D and centre (forward.cu:215-236,
    auxiliary.h:48-58), in fp32;
  * must_keep(): per tile of a rectangle, whether some pixel centre inside the image passes the blend kernels' accept test in THEIR
    arithmetic -- fp32, the order of gsr_pair_power (render_common.h), d = mean - pixel;
  * the needle family and the ordinary family of tests/test_trim_needles_cpu.py, and the 3D construction of the needles for
    tests/test_trim_needles_gpu.py and tools/trim_stress.py.
"""
import math

import numpy as np

F = np.float32
TILE = 16
GROUPS, MAX_UNITS = 8, 3
K1, K2 = F(2.0), F(4.0)          # GSR_TRIM_K1, GSR_TRIM_K2
EPS = F(2.0 ** -23)


def col_shift(w):
    return 0 if w <= 8 else (w - 1).bit_length() - 3


def row_shift(h):
    return 0 if h <= 16 else (h - 1).bit_length() - 4


def rect_pack(x0, y0, w, h):
    return 0xFFFFFFFF if (w == 0 or h == 0) else (x0 | (y0 << 8) | ((w - 1) << 16) | ((h - 1) << 24))


def _rcp(x):
    return F(1.0) / x


def _log(x):
    return F(np.log(np.float64(x)))


def _sqrt(x):
    return np.sqrt(x)   # (of an np.float32: correctly rounded, NaN below zero)


def rect_trim(px, py, ca, cb, cc, opacity, x0, y0, w, h):
    """gsr_rect_trim(): the trim word of one Gaussian.  px .. opacity: np.float32 scalars, the rectangle in tiles."""
    px, py, ca, cb, cc, opacity = (F(v) for v in (px, py, ca, cb, cc, opacity))
    if w <= 0 or h <= 0:
        return 0
    cs, rs = col_shift(w), row_shift(h)
    groups = (w + (1 << cs) - 1) >> cs
    with np.errstate(all="ignore"):
        det0 = ca * cc - cb * cb
        dspan = (K1 * EPS) * (ca * cc + cb * cb)
        det = det0 - dspan
        X = np.fmax(abs(F(x0 * TILE) - px), abs(F((x0 + w) * TILE - 1) - px))
        Y = np.fmax(abs(F(y0 * TILE) - py), abs(F((y0 + h) * TILE - 1) - py))
        tau0 = F(2.0) * _log(F(255.0) * opacity) * F(1.001) + F(0.01)
        tau = tau0 + (K2 * EPS) * (ca * X * X + F(2.0) * abs(cb) * X * Y + cc * Y * Y)
        if not (det > 0) or not (ca > 0) or not (cc > 0) or not (tau == tau):
            return 0
        trim = 0
        first, last = groups, 0
        if tau0 > 0:
            inv_det = _rcp(det)
            ex = _sqrt(tau * cc * inv_det) * F(1.0001) + F(0.01)
            eyy = _sqrt(tau * ca * inv_det) * F(1.0001) + F(0.01)
            xs = abs(cb) * _sqrt(tau * inv_det * _rcp(ca))
            xs1 = xs * F(1.0001) + F(0.01)
            xs0 = xs * (det * _rcp(det0 + dspan)) * F(0.9999) - F(0.01)
            bx0, bx1 = (xs0, xs1) if cb <= 0 else (-xs1, -xs0)
            inv_cc = _rcp(cc)
            for c in range(groups):
                c0, c1 = x0 + (c << cs), min(x0 + w, x0 + ((c + 1) << cs))
                lo = F(c0 * TILE) - px - F(0.01)
                hi = F(c1 * TILE - 1) - px + F(0.01)
                t = b = MAX_UNITS
                if not (lo > ex) and not (hi < -ex):
                    lo, hi = np.fmax(lo, -ex), np.fmin(hi, ex)
                    rlo = _sqrt(np.fmax(F(0.0), tau * cc - det * lo * lo))
                    rhi = _sqrt(np.fmax(F(0.0), tau * cc - det * hi * hi))
                    ymax = np.fmax((-cb * lo + rlo) * inv_cc, (-cb * hi + rhi) * inv_cc)
                    ymin = np.fmin((-cb * lo - rlo) * inv_cc, (-cb * hi - rhi) * inv_cc)
                    if lo <= bx1 and bx0 <= hi:
                        ymax = eyy
                    if lo <= -bx0 and -bx1 <= hi:
                        ymin = -eyy
                    ymax = ymax * F(1.0001) + F(0.01)
                    ymin = ymin * F(1.0001) - F(0.01)
                    r0 = np.floor((py + ymin) * F(1.0 / TILE))
                    r1 = np.floor((py + ymax) * F(1.0 / TILE))
                    unit = F(1.0 / (1 << rs))
                    tf = np.fmin(np.floor(np.fmax(r0 - F(y0), F(0.0)) * unit), F(MAX_UNITS))
                    bf = np.fmin(np.floor(np.fmax(F(y0 + h - 1) - r1, F(0.0)) * unit), F(MAX_UNITS))
                    t, b = int(tf), int(bf)
                trim |= (t | (b << 2)) << (4 * c)
                if ((t + b) << rs) < h:
                    first, last = min(first, c), c + 1
        else:
            for c in range(groups):
                trim |= 15 << (4 * c)
        for c in range(GROUPS):
            if first < c and c + 1 < last:
                nib = (trim >> (4 * c)) & 15
                if (((nib & 3) + (nib >> 2)) << rs) >= h:
                    trim &= ~(15 << (4 * c))
    return trim & 0xFFFFFFFF


def conic_radius_rect(cov, px, py, W, H):
    """The reference's conic (a, b, c), radius and tile rectangle (x0, y0, w, h) of a splat with cov2D = (cxx, cxy, cyy) -- the
    0.3 of the low-pass filter already inside -- centred at pixel (px, py): forward.cu:215-236, auxiliary.h:48-58, in fp32.
    None if the reference drops the splat."""
    cx, cy, cz = (F(v) for v in cov)
    px, py = F(px), F(py)
    det = cx * cz - cy * cy
    if det == 0:
        return None
    det_inv = F(1.0) / det
    conic = (cz * det_inv, -cy * det_inv, cx * det_inv)
    mid = F(0.5) * (cx + cz)
    lam1 = mid + np.sqrt(np.fmax(F(0.1), mid * mid - det))
    lam2 = mid - np.sqrt(np.fmax(F(0.1), mid * mid - det))
    radius = int(np.ceil(F(3.0) * np.sqrt(np.fmax(lam1, lam2))))
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    r = F(radius)   # (the reference adds the int to the float: a float sum; the division by the block size in float; truncation)
    x0 = min(gx, max(0, int((px - r) / F(TILE))))
    y0 = min(gy, max(0, int((py - r) / F(TILE))))
    x1 = min(gx, max(0, int((px + r + F(TILE - 1)) / F(TILE))))
    y1 = min(gy, max(0, int((py + r + F(TILE - 1)) / F(TILE))))
    if (x1 - x0) * (y1 - y0) == 0:
        return None
    return conic, radius, (x0, y0, x1 - x0, y1 - y0)


def must_keep(px, py, ca, cb, cc, opacity, rect, W, H):
    """The blend kernels' accept test at every pixel centre of the rectangle that lies inside the image, in their arithmetic:
    d = mean - pixel, power = ((a dx) dx + (c dy) dy) * -0.5 - (b dx) dy in fp32, nothing fused; exp in float64 of that fp32 power.
    Returns, per tile (h, w): `must` -- some pixel has power <= 0 and opacity exp(power) >= (1 + 1e-5) / 255, the tile has to be in
    the list; `score` -- the largest power + ln(255 opacity) over the tile's pixels with power <= 0 (>= 0: reaches alpha = 1 / 255;
    -inf: no pixel with power <= 0); and the largest ca dx^2 + 2 |cb dx dy| + cc dy^2 over all these pixels (float64)."""
    x0, y0, w, h = rect
    a, b, c, mx, my = F(ca), F(cb), F(cc), F(px), F(py)
    xs = np.arange(x0 * TILE, (x0 + w) * TILE)
    ys = np.arange(y0 * TILE, (y0 + h) * TILE)
    dx, dy = mx - xs.astype(F), my - ys.astype(F)
    ax2, bdx, cy2 = (a * dx) * dx, b * dx, (c * dy) * dy
    power = (ax2[None, :] + cy2[:, None]) * F(-0.5) - bdx[None, :] * dy[:, None]
    assert power.dtype == F
    inside = (xs < W)[None, :] & (ys < H)[:, None]
    o = np.float64(F(opacity))
    with np.errstate(all="ignore"):
        p64 = power.astype(np.float64)
        ok = inside & (power <= 0)
        hit = ok & (o * np.exp(p64) >= (1.0 + 1e-5) / 255.0)
        score = np.where(ok, p64 + (np.log(255.0 * o) if o > 0 else -np.inf), -np.inf)
    tiles = lambda v: v.reshape(h, TILE, w, TILE)
    d64x, d64y = dx.astype(np.float64)[xs < W], dy.astype(np.float64)[ys < H]
    X, Y = np.abs(d64x).max(), np.abs(d64y).max()
    mag = float(a) * X * X + 2.0 * abs(float(b)) * X * Y + float(c) * Y * Y
    return tiles(hit).any(axis=(1, 3)), tiles(score).max(axis=(1, 3)), mag


def kept_tiles(trim, rect, gx):
    """(h, w) bool: the tiles of the rectangle that the binning keeps for this trim word (util.trim_kept: the decoder's restatement)."""
    import util
    x0, y0, w, h = rect
    rshape = np.array([[rect_pack(x0, y0, w, h), trim]], dtype=np.uint32)
    ty, tx = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), indexing="ij")
    t = (ty * gx + tx).reshape(-1)
    return util.trim_kept(rshape, np.zeros(t.shape, np.int64), t, gx).reshape(h, w)


# ---- the families ----
NEEDLE_L = (400.0, 700.0, 1000.0, 1500.0)
NEEDLE_THETA = (30.0, 40.0, 45.0, 50.0, 60.0, 135.0)
NEEDLE_OPACITY = (0.99, 0.3, 0.02)
NEEDLE_K = (1.0, -1.0, 2.0, -2.0, 2.8, -2.8)
NEEDLE_ANCHOR = ((0.5, 0.5), (0.22, 0.71))   # the points of the image (fractions of W, H) the long axes pass through
NEEDLE_THIN = 0.3                            # the thin axis's variance: what the low-pass filter leaves of a line


def needle_cases():
    """(L, theta in degrees, opacity, k, anchor): 864 of them."""
    return [(L, th, o, k, an) for L in NEEDLE_L for th in NEEDLE_THETA for o in NEEDLE_OPACITY for k in NEEDLE_K for an in NEEDLE_ANCHOR]


def needle_2d(case, W, H):
    """cov2D = R(theta) diag(L^2, 0.3) R(theta)^T and the centre, k L along the long axis from the anchor (float64; the callers cast)."""
    L, th, o, k, an = case
    c, s = math.cos(math.radians(th)), math.sin(math.radians(th))
    l1, l2 = L * L, NEEDLE_THIN
    cov = (c * c * l1 + s * s * l2, c * s * (l1 - l2), s * s * l1 + c * c * l2)
    ax, ay = an[0] * W + 0.3, an[1] * H - 0.2
    return cov, ax + k * L * c, ay + k * L * s


def needle_3d(cases, cam, depth=4.0):
    """The same needles as 3D Gaussians in the plane of view depth `depth` in front of gsr_scene.make_camera(W, H) (camera at
    (0, 0, -4), looking down +z: world z = depth - 4): scales (long, 1e-4, 1e-4), rotated about the view axis by theta, so that
    the 2D quantities land near needle_2d()'s (a needle inside a plane of constant depth sees only the Jacobian's focal / depth
    part, so the clamp of forward.cu:84-89 at the centres far off the image does not bend it).  What the tests decide from is
    what the device wrote, not this.  Returns means3D (n, 3), scales (n, 3), rotations (n, 4), opacities (n, 1) as float32 arrays."""
    W, H = cam.image_width, cam.image_height
    fx, fy = W / (2.0 * cam.tanfovx), H / (2.0 * cam.tanfovy)
    n = len(cases)
    means, scales, rots, ops = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 4)), np.zeros((n, 1))
    for i, case in enumerate(cases):
        L, th, o, k, an = case
        _, px, py = needle_2d(case, W, H)
        means[i] = ((px + 0.5 - W / 2.0) * depth / fx, (py + 0.5 - H / 2.0) * depth / fy, depth - 4.0)
        scales[i] = (L * depth / fx, 1e-4, 1e-4)
        rots[i] = (math.cos(math.radians(th) / 2.0), 0.0, 0.0, math.sin(math.radians(th) / 2.0))   # (w, x, y, z): about z
        ops[i] = o
    return means.astype(F), scales.astype(F), rots.astype(F), ops.astype(F)


def ordinary_cases(n, W, H, seed=0):
    """n ordinary splats: long axis 2 .. 60 px (log-uniform), any aspect down to the low-pass floor, any angle, opacity from
    the threshold up, centre in or near the image.  Yields (cov2D, px, py, opacity)."""
    r = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        L = math.exp(r.uniform(math.log(2.0), math.log(60.0)))
        l1 = L * L
        l2 = max(NEEDLE_THIN, l1 * math.exp(r.uniform(math.log(1e-3), 0.0)))
        th = r.uniform(0.0, math.pi)
        c, s = math.cos(th), math.sin(th)
        cov = (c * c * l1 + s * s * l2, c * s * (l1 - l2), s * s * l1 + c * c * l2)
        o = float(r.choice([r.uniform(0.0, 1.0), math.exp(r.uniform(math.log(1.0 / 255.0), 0.0)), 1.0]))
        out.append((cov, r.uniform(-40.0, W + 40.0), r.uniform(-40.0, H + 40.0), o))
    return out
