"""Fixtures and a numpy reference for the seam tests of the depth sort and the binning (tests/test_binning_seams_cpu.py,
tests/test_binning_seams_gpu.py).  No GPU code.

The chain under test (csrc/preprocess.hip scans, sort.hip, depthsort.hip, tilebin.hip, binning.hip) turns per-Gaussian depth bits
and tile rectangles into the sorted instance list and the tile ranges: integers throughout.  Its kernels are built from fixed-size
pieces ("Seams of the binning chain"); the fixtures here put a count exactly on, one below and one above each
of them.  Every fixture is made of Gaussians whose rectangle is known by construction:

  scale 1e-4 (radius 3 px) at a tile centre (16 i + 7.5, 16 j + 7.5)      1 tile
                          on a vertical seam (16 i - 0.5, 16 j + 7.5)     2 tiles: 2 columns x 1 row
                          at a corner (16 i - 0.5, 16 j - 0.5)            4 tiles
  scales (s, s, 1e-4) with s from radius_scale()                           a radius of exactly r px

and the camera is always make_camera()'s default pose (at (0, 0, -4), looking down +z), where the view depth is z + 4 whatever x
and y are, and that sum is exact in fp32 for the depths used: the fixture chooses the depth BITS.

The reference (reference_binning) follows the reference's duplicateWithKeys + SortPairs + identifyTileRanges
(rasterizer_impl.cu:78-126, 357-374, 133-162) in numpy; it depends neither on the HIP code nor on the C oracle."""
import functools
import math
import re
from typing import NamedTuple, Optional

import numpy as np
import torch

import gsr_scene

CULLED = np.uint32(0xFFFFFFFF)
F32_4 = 0x40800000   # bits of 4.0f
F32_2_5 = 0x40200000  # bits of 2.5f
F32_5_5 = 0x40B00000  # bits of 5.5f


class Case(NamedTuple):
    name: str
    scene: gsr_scene.Scene      # (shs is a dummy: the cases run with colors_precomp at degree 0)
    colors: torch.Tensor        # (P, 3)
    cam: gsr_scene.Camera
    bits: Optional[np.ndarray]  # chosen depth bits per Gaussian, CULLED for the ones behind the camera (None: a random scene, group F)
    expect: dict                # what the name promises (test_binning_seams_cpu.py asserts it on the oracle's state)

    @property
    def P(self):
        return int(self.scene.means3D.shape[0])


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def place(cam, px, py, depth):
    """World positions (n, 3) float32 that project to pixel coordinates (px, py) at view depth `depth`, with the reference's pixel
    convention pix = ((ndc + 1) * S - 1) / 2 (auxiliary.h:44)."""
    px, py, depth = (np.asarray(v, np.float64) for v in (px, py, depth))
    ndcx = (2.0 * px + 1.0) / cam.image_width - 1.0
    ndcy = (2.0 * py + 1.0) / cam.image_height - 1.0
    view = np.stack([ndcx * cam.tanfovx * depth, ndcy * cam.tanfovy * depth, depth, np.ones_like(depth)], axis=-1)
    world = view @ np.linalg.inv(cam.world_view_transform.numpy().astype(np.float64))   # (row vectors: view = world @ W2C^T)
    return world[..., :3].astype(np.float32)


def radius_scale(cam, depth, r):
    """Scale s such that a Gaussian with scales (s, s, 1e-4), identity rotation, at view depth `depth` gets the radius
    ceil(3 sqrt(lambda1)) = r px exactly: its screen covariance is diag(sigma^2, sigma^2) + 0.3 up to 1e-8 sigma^2 whatever its position
    (the flat z axis takes the perspective term out), and 3 sigma = r - 0.5 sits half a pixel from the two roundings next to it."""
    focal = cam.image_width / (2.0 * cam.tanfovx)
    return (r - 0.5) / 3.0 * np.asarray(depth, np.float64) / focal


def centres(i, j):
    return 16.0 * np.asarray(i) + 7.5, 16.0 * np.asarray(j) + 7.5


def seams(i, j):
    return 16.0 * np.asarray(i) - 0.5, 16.0 * np.asarray(j) + 7.5


def corners(i, j):
    return 16.0 * np.asarray(i) - 0.5, 16.0 * np.asarray(j) - 0.5


def uniform_bits(rng, n, lo=2.5, hi=5.5):
    return rng.uniform(lo, hi, n).astype(np.float32).view(np.uint32)


def make_case(name, cam, px, py, bits, expect, scales=1e-4, opacity=0.9, seed=0):
    bits = np.asarray(bits, np.uint32)
    P = bits.shape[0]
    vis = bits != CULLED
    depth = np.where(vis, bits.view(np.float32).astype(np.float64), -1.0)   # culled: one unit behind the camera
    means = place(cam, np.asarray(px, np.float64) * np.ones(P), np.asarray(py, np.float64) * np.ones(P), depth)
    sc = np.empty((P, 3), np.float32)
    sc[:] = scales      # a scalar or (P, 3)
    rot = np.zeros((P, 4), np.float32)
    rot[:, 0] = 1.0
    op = np.empty((P, 1), np.float32)
    op[:] = opacity     # a scalar or (P, 1)
    g = torch.Generator().manual_seed(seed)
    colors = torch.rand(P, 3, generator=g)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    scene = gsr_scene.Scene(t(means), t(sc), t(rot), t(op), torch.zeros(P, 1, 3), torch.tensor([0.1, 0.2, 0.3]))
    exp = dict(P=P, visible=int(vis.sum()), culled=int(P - vis.sum()))
    exp.update(expect)
    return Case(name, scene, colors, cam, bits, exp)


# ---- the numpy reference -----------------------------------------------------------------------------------------------------------
def reference_depth_order(depth_bits):
    return np.argsort(np.asarray(depth_bits, np.uint32), kind="stable").astype(np.uint32)


def depth_buckets(depth_bits):
    """numpy restatement of gsr_key_bias_of (csrc/gsr_depth_key.h): min, range and top_shift of the visible keys and the top-digit
    bucket of each of them.  Only used to assert that a fixture has the bucket sizes its name says."""
    k = np.asarray(depth_bits, np.uint32)
    k = k[k != CULLED].astype(np.int64)
    mn, vr = (int(k.min()), int(k.max() - k.min())) if k.size else (0, 0)
    s = max(vr.bit_length() - 8, 0)
    if (vr >> s) >= 255:
        s += 1
    bucket = (k - mn) >> s
    return dict(min=mn, range=vr, top_shift=s, bucket=bucket, sizes=np.bincount(bucket, minlength=256))


def rect_of_state(rect_words, tiles_touched):
    """(P, 4) int64 {x0, y0, w, h} from the library's GsrGeometry::rect words {x | y << 16, w | h << 16}; w = h = 0 where nothing is touched."""
    r = np.asarray(rect_words).astype(np.int64)
    out = np.stack([r[:, 0] & 0xFFFF, r[:, 0] >> 16, r[:, 1] & 0xFFFF, r[:, 1] >> 16], axis=1)
    out[np.asarray(tiles_touched) == 0] = 0
    return out


def rect_of_oracle(o):
    """The same from the oracle's means2D and radii: getRect (auxiliary.h:46-58) in fp32."""
    gx, gy = (o["W"] + 15) // 16, (o["H"] + 15) // 16
    m, r = o["means2D"].astype(np.float32), o["radii"].astype(np.float32)
    f = lambda v, g: np.clip((v / np.float32(16.0)).astype(np.int32), 0, g).astype(np.int64)
    x0, y0 = f(m[:, 0] - r, gx), f(m[:, 1] - r, gy)
    x1, y1 = f(m[:, 0] + r + np.float32(15.0), gx), f(m[:, 1] + r + np.float32(15.0), gy)
    out = np.stack([x0, y0, x1 - x0, y1 - y0], axis=1)
    out[o["radii"] <= 0] = 0
    return out


def reference_binning(rect, depth_bits, gx, gy):
    """Instances of every Gaussian in index order, y outer and x inner, key = tile << 32 | depth bits, stable sort, tile ranges
    ((0, 0) for tiles without instances)."""
    rect = np.asarray(rect, np.int64)
    bits = np.asarray(depth_bits, np.uint32)
    x0, y0, w, h = rect.T
    n = w * h
    R = int(n.sum())
    g = np.repeat(np.arange(rect.shape[0], dtype=np.int64), n)
    local = np.arange(R, dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    tile = (y0[g] + local // np.maximum(w[g], 1)) * gx + x0[g] + local % np.maximum(w[g], 1)
    key = (tile.astype(np.uint64) << np.uint64(32)) | bits[g].astype(np.uint64)
    order = np.argsort(key, kind="stable")
    keys = key[order]
    st = (keys >> np.uint64(32)).astype(np.int64)
    T = gx * gy
    lo, hi = np.searchsorted(st, np.arange(T), "left"), np.searchsorted(st, np.arange(T), "right")
    ranges = np.where((hi > lo)[:, None], np.stack([lo, hi], 1), 0).astype(np.uint32)
    return dict(point_list=g[order].astype(np.uint32), keys=keys, ranges=ranges)


def trimmed(want, rshape, gx, gy):
    """The reference lists less the instances the trim words name (util.trim_kept), as util.trimmed_expectation forms them."""
    import util
    tile_of = (want["keys"] >> np.uint64(32)).astype(np.int64)
    kept = util.trim_kept(rshape, want["point_list"], tile_of, gx, gy)
    kcum = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    rng = want["ranges"].astype(np.int64)
    new_len = kcum[rng[:, 1]] - kcum[rng[:, 0]]
    new_start = kcum[rng[:, 0]]
    ranges = np.where((new_len > 0)[:, None], np.stack([new_start, new_start + new_len], 1), 0).astype(np.uint32)
    return dict(point_list=want["point_list"][kept], keys=want["keys"][kept], ranges=ranges)


def check_lists(got, want, label=""):
    """The one comparison of all groups: point_list, keys and ranges must be equal arrays.  Raises AssertionError naming the first
    differing position and its tile."""
    for k in ("point_list", "keys"):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        n = min(a.shape[0], b.shape[0])
        d = np.nonzero(a[:n] != b[:n])[0]
        if d.size or a.shape[0] != b.shape[0]:
            p = int(d[0]) if d.size else n
            src = want["keys"] if p < len(want["keys"]) else got["keys"]
            tile = int(np.asarray(src)[min(p, len(src) - 1)] >> np.uint64(32)) if len(src) else -1
            ga = int(a[p]) if p < a.shape[0] else None
            wa = int(b[p]) if p < b.shape[0] else None
            raise AssertionError(f"{label}: {k} has {a.shape[0]} entries, expected {b.shape[0]}; first difference at position {p} "
                                 f"(tile {tile}): got {ga}, expected {wa}; {int(d.size)} positions differ")
    a, b = np.asarray(got["ranges"]).astype(np.int64), np.asarray(want["ranges"]).astype(np.int64)
    if a.shape != b.shape:
        raise AssertionError(f"{label}: ranges of {a.shape[0]} tiles, expected {b.shape[0]}")
    d = np.nonzero((a != b).any(axis=1))[0]
    if d.size:
        t = int(d[0])
        raise AssertionError(f"{label}: range of tile {t} is {tuple(a[t])}, expected {tuple(b[t])}; {int(d.size)} tiles differ")


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def _rotation(P, gx, gy):
    """Tile centres, vertical seams and corners in rotation (1, 2, 4 tiles): pixel coordinates and tiles touched."""
    i = np.arange(P)
    kind = i % 3
    ti, tj = 1 + (i // 3) % (gx - 1), 1 + (i // 7) % (gy - 1)
    cx, cy = centres(ti, tj)
    sx, sy = seams(ti, tj)
    kx, ky = corners(ti, tj)
    px = np.where(kind == 0, cx, np.where(kind == 1, sx, kx))
    py = np.where(kind == 0, cy, np.where(kind == 1, sy, ky))
    return px, py, np.array([1, 2, 4])[kind]


A_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, 65535, 65536, 65537)
A_NAMES = [f"A_{P}_{v}" for P in A_COUNTS for v in ("all", "fifth")] + [f"A_9000_culled{n}" for n in (2047, 2048, 2049)]


def _case_A(name):
    _, P, v = name.split("_")
    P = int(P)
    rng = np.random.default_rng(P * 7 + len(v))
    cam = gsr_scene.make_camera(64, 48)
    bits = uniform_bits(rng, P)
    if v == "fifth":
        bits[4::5] = CULLED
    elif v.startswith("culled"):
        bits[rng.choice(P, int(v[6:]), replace=False)] = CULLED
    px, py, tt = _rotation(P, 4, 3)
    vis = bits != CULLED
    exp = dict(kinds={k: int((tt[vis] == k).sum()) for k in (1, 2, 4)}, R=int(tt[vis].sum()))
    if v.startswith("culled"):
        exp["culled"] = int(v[6:])
    elif v == "fifth":
        exp["culled"] = P // 5
    else:
        exp["culled"] = 0
    return make_case(name, cam, px, py, bits, exp, seed=P)


B_SLAB = 0x60     # the top-digit bucket that starts at depth 4.0 when the smallest visible depth is 2.5 and top_shift is 16
B_NAMES = ([f"B_distinct{n}" for n in (2047, 2048, 2049, 12287, 12288, 12289)] + ["B_digit2048", "B_digit2049", "B_identical2049"] +
           [f"B_parts{n}" for n in (3200, 3201, 4800, 4801)] + ["B_flat5000"])


def _case_B(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    cam = gsr_scene.make_camera(64, 48)
    if name == "B_flat5000":   # the whole depth range is under 255 float steps: top_shift = 0, nothing left to sort below the top digit
        off = rng.integers(0, 200, 5000)
        off[:2] = (0, 199)
        bits = (F32_4 + rng.permutation(off)).astype(np.uint32)
        exp = dict(top_shift=0, range=199)
    else:
        back = np.concatenate([uniform_bits(rng, 1500, 2.5, 3.5), uniform_bits(rng, 1500, 4.5, 5.5)])
        back[0], back[1] = F32_2_5, F32_5_5   # pins the minimum and the range: top_shift = 16, bucket edges on multiples of 65 536 float steps
        kind = name[2:]
        if kind.startswith("distinct") or kind.startswith("parts"):
            n = int(re.fullmatch(r"(?:distinct|parts)(\d+)", kind).group(1))
            slab = F32_4 + rng.choice(65536, n, replace=False)
        elif kind.startswith("digit"):   # m keys inside one next-digit value (256 float steps), the rest of the 6 000 elsewhere in the bucket
            m = int(kind[5:])
            inside = F32_4 + 0x3700 + rng.integers(0, 256, m)
            pool = np.setdiff1d(np.arange(65536), np.arange(0x3700, 0x3800))
            slab = np.concatenate([inside, F32_4 + rng.choice(pool, 6000 - m, replace=False)])
            exp_digit = m
        else:                            # 2 049 identical keys among the 6 000
            slab = np.concatenate([np.full(2049, F32_4 + 0x5A5A), F32_4 + rng.choice(np.setdiff1d(np.arange(65536), [0x5A5A]), 6000 - 2049, replace=False)])
        bits = rng.permutation(np.concatenate([back, slab.astype(np.uint32)]).astype(np.uint32))
        exp = dict(top_shift=16, range=F32_5_5 - F32_2_5, slab=(B_SLAB, len(slab)))
        if kind.startswith("digit"):
            exp["digit"] = (0x37, exp_digit)
        if kind.startswith("identical"):
            exp["identical"] = (F32_4 + 0x5A5A, 2049)
    px, py, tt = _rotation(len(bits), 4, 3)
    exp.update(kinds={k: int((tt == k).sum()) for k in (1, 2, 4)}, R=int(tt.sum()), culled=0)
    return make_case(name, cam, px, py, bits, exp, seed=len(bits))


def _mixed(rng, gx, gy, n1, n2, n4):
    """n1 single-tile, n2 two-column and n4 four-tile Gaussians at random tiles of a gx x gy grid of full tiles, shuffled."""
    px = np.concatenate([centres(rng.integers(0, gx, n1), 0)[0], seams(rng.integers(1, gx, n2), 0)[0], corners(rng.integers(1, gx, n4), 0)[0]])
    py = np.concatenate([centres(0, rng.integers(0, gy, n1))[1], seams(0, rng.integers(0, gy, n2))[1], corners(0, rng.integers(1, gy, n4))[1]])
    tt = np.concatenate([np.full(n1, 1), np.full(n2, 2), np.full(n4, 4)])
    p = rng.permutation(n1 + n2 + n4)
    return px[p], py[p], tt[p]


def _col_pairs(px, tt, gx):
    """Column pairs per tile column of single-tile / seam / corner Gaussians (a seam or corner at 16 i - 0.5 touches columns i - 1 and i)."""
    c = np.floor(np.asarray(px) / 16.0).astype(np.int64)   # seams and corners: floor((16 i - 0.5) / 16) = i - 1
    cnt = np.bincount(c, minlength=gx)
    two = np.asarray(tt) > 1
    return cnt + np.bincount(c[two] + 1, minlength=gx)[:gx]


C1_NAMES = [f"C1_{P}" for P in (1023, 1024, 1025)]
C2_NAMES = [f"C2_pairs{n}" for n in (1023, 1024, 1025, 65535, 65536, 65537)]
C3_NAMES = [f"C3_{where}_{1024 * k + d}" for where in ("mid", "col0", "col255") for k in (1, 2) for d in (-1, 0, 1)]
C4_NAMES = ["C4_strip_w256", "C4_strip_w255", "C4_column_h256", "C4_column_h255"]
C5_NAMES = ["C5_trim_words"]


def _case_C1(name):
    P = int(name[3:])
    rng = np.random.default_rng(P)
    cam = gsr_scene.make_camera(256, 256)
    px, py, tt = _mixed(rng, 16, 16, P, 0, 0)
    return make_case(name, cam, px, py, uniform_bits(rng, P), dict(kinds={1: P, 2: 0, 4: 0}, pairs=P, R=P, culled=0), seed=P)


def _case_C2(name):
    pairs = int(name[8:])
    rng = np.random.default_rng(pairs)
    cam = gsr_scene.make_camera(256, 256)
    n2, n4 = pairs // 5, pairs // 8
    n1 = pairs - 2 * (n2 + n4)
    px, py, tt = _mixed(rng, 16, 16, n1, n2, n4)
    exp = dict(kinds={1: n1, 2: n2, 4: n4}, pairs=pairs, R=n1 + 2 * n2 + 4 * n4, culled=0, col_pairs=_col_pairs(px, tt, 16))
    return make_case(name, cam, px, py, uniform_bits(rng, len(px)), exp, seed=pairs)


def _case_C3(name):
    _, where, n = name.split("_")
    n = int(n)
    rng = np.random.default_rng(n + len(where))
    if where == "mid":   # column 7 holds n pairs, its neighbours 6 and 8 and the far columns 2 and 12 one each, the rest none
        cam, gx, gy = gsr_scene.make_camera(256, 256), 16, 16
        cols = np.concatenate([np.full(n, 7), [6, 8, 2, 12]])
    else:                # everything in the first / last tile column of a 4096 x 16 strip
        cam, gx, gy = gsr_scene.make_camera(4096, 16), 256, 1
        cols = np.full(n, 0 if where == "col0" else 255)
    cols = rng.permutation(cols)
    px, py = centres(cols, rng.integers(0, gy, len(cols)))
    want = np.bincount(cols, minlength=gx)
    exp = dict(kinds={1: len(cols), 2: 0, 4: 0}, pairs=len(cols), R=len(cols), culled=0, col_pairs=want)
    return make_case(name, cam, px, py, uniform_bits(rng, len(cols)), exp, seed=n)


def _case_C4(name):
    """70 depth-consecutive splats of 256 (255) tiles in a row among 500 small ones: the 64 segments of one wave then expand to
    64 * 256 = 16 384 elements."""
    _, shape, span = name.split("_")
    span = int(span[1:])
    rng = np.random.default_rng(span + len(shape))
    strip = shape == "strip"
    cam = gsr_scene.make_camera(4096, 16) if strip else gsr_scene.make_camera(16, 4096, fovx=2.0 * math.atan(math.tan(0.5) / 256.0))
    nbig, nsmall = 70, 500
    # the big ones: consecutive floats from 4.0 on; the small ones: anywhere but there
    small_bits = np.concatenate([uniform_bits(rng, nsmall // 2, 2.5, 3.9), uniform_bits(rng, nsmall - nsmall // 2, 4.1, 5.5)])
    big_bits = (F32_4 + rng.permutation(nbig)).astype(np.uint32)
    along_small, _ = centres(rng.integers(0, 256, nsmall), 0)
    # radius 2500 px: centred at 2048 the rectangle is clipped to all 256 tiles; centred at 1572.5 its far edge 4072.5 + 15 lies in tile 255
    # exclusive, so it spans tiles 0 .. 254
    along_big = np.full(nbig, 2048.0 if span == 256 else 1572.5)
    along = np.concatenate([along_small, along_big])
    across = np.full(nsmall + nbig, 7.5)
    bits = np.concatenate([small_bits, big_bits])
    s_big = radius_scale(cam, big_bits.view(np.float32), 2500)
    scales = np.full((nsmall + nbig, 3), 1e-4)
    scales[nsmall:, 0] = scales[nsmall:, 1] = s_big
    p = rng.permutation(nsmall + nbig)
    px, py = (along[p], across[p]) if strip else (across[p], along[p])
    exp = dict(kinds={1: nsmall, span: nbig}, R=nsmall + span * nbig, pairs=(nsmall + span * nbig) if strip else (nsmall + nbig), culled=0,
               consecutive=(nbig, span))
    return make_case(name, cam, px, py, bits[p], exp, scales=scales[p], seed=span)


C5_SHAPES = [(w, h) for w in (8, 9, 16, 17) for h in (16, 17, 32, 33)]
_C5_RADIUS = {16: 120, 17: 128, 32: 248, 33: 256}   # a radius r gives n = floor((2 r + 23) / 16) tiles when the near edge sits 8 px inside a tile


def _case_C5(name):
    """Rectangles of exactly 8, 9, 16 and 17 columns by 16, 17, 32 and 33 rows on 1056 x 560 (66 x 35 tiles): the reference's rectangle is
    the square of one radius (n x n tiles, n the larger of the two), so the smaller count is cut by the image's left / top edge.  Each
    at opacity 0.9 and 2/255."""
    rng = np.random.default_rng(5)
    cam = gsr_scene.make_camera(1056, 560)
    nsmall = 300
    px, py, r, op = [], [], [], []
    for w, h in C5_SHAPES:
        for o in (0.9, 2.0 / 255.0):
            n = max(w, h)
            rr = _C5_RADIUS[n]
            # cut: far edge at 16 k + 8 - 15, the near edge then lies left of / above pixel 16 (tile 0, or clipped); whole: near edge in
            # the middle of tile 1
            px.append(16.0 * w - 7.0 - rr if w < n else 24.0 + rr)
            py.append(16.0 * h - 7.0 - rr if h < n else 24.0 + rr)
            r.append(rr); op.append(o)
    nbig = len(px)
    sx, sy, _ = _mixed(rng, 66, 35, nsmall, 0, 0)
    bits = uniform_bits(rng, nsmall + nbig)
    scales = np.full((nsmall + nbig, 3), 1e-4)
    scales[nsmall:, 0] = scales[nsmall:, 1] = radius_scale(cam, bits[nsmall:].view(np.float32), np.array(r))
    opac = np.concatenate([np.where(np.arange(nsmall) % 2 == 0, 0.9, 2.0 / 255.0), op]).reshape(-1, 1)
    p = rng.permutation(nsmall + nbig)
    shapes = np.concatenate([np.ones((nsmall, 2), np.int64), np.repeat(np.array(C5_SHAPES), 2, axis=0)])[p]
    exp = dict(shapes=shapes, R=int((shapes[:, 0] * shapes[:, 1]).sum()), pairs=int(shapes[:, 0].sum()), culled=0)
    return make_case(name, cam, np.concatenate([sx, px])[p], np.concatenate([sy, py])[p], bits[p], exp, scales=scales[p], opacity=opac[p], seed=5)


D1_COUNTS = (1, 2, 3, 5, 2047, 2048, 2049, 131071, 131072, 131073)
D1_NAMES = [f"D1_R{R}" for R in D1_COUNTS]
D2_NAMES = ["D2_tile0", "D2_last_tile", "D2_middle_third"]
D3_NAMES = ["D3_256_tiles", "D3_257_tiles"]
D4_NAME = "D4_u32_tile_ids"
D4_W, D4_H = 524304, 17   # 32 769 x 2 = 65 538 tiles


def _case_D1(name):
    R = int(name[4:])
    rng = np.random.default_rng(R)
    cam = gsr_scene.make_camera(64, 48)
    n4, n2 = R // 6, R // 12
    n1 = R - 4 * n4 - 2 * n2
    px, py, tt = _mixed(rng, 4, 3, n1, n2, n4)
    return make_case(name, cam, px, py, uniform_bits(rng, len(px)), dict(kinds={1: n1, 2: n2, 4: n4}, R=R, culled=0), seed=R)


def _case_D2(name):
    rng = np.random.default_rng(len(name))
    cam = gsr_scene.make_camera(256, 256)
    P = 2000
    if name == "D2_tile0":
        ti, tj, tiles = np.zeros(P, np.int64), np.zeros(P, np.int64), (0, 0)
    elif name == "D2_last_tile":
        ti, tj, tiles = np.full(P, 15), np.full(P, 15), (255, 255)
    else:   # tiles 86 .. 169 of 256: the first and the last third stay empty
        t = rng.integers(86, 170, P)
        t[:2] = (86, 169)
        ti, tj, tiles = t % 16, t // 16, (86, 169)
    px, py = centres(ti, tj)
    return make_case(name, cam, px, py, uniform_bits(rng, P), dict(kinds={1: P, 2: 0, 4: 0}, R=P, culled=0, tile_span=tiles), seed=P)


def _case_D3(name):
    rng = np.random.default_rng(len(name) + 3)
    gx = 16 if name == "D3_256_tiles" else 257   # 256 tiles: 8 bits of tile id, one sort pass; 257: nine bits, two passes
    cam = gsr_scene.make_camera(256, 256) if gx == 16 else gsr_scene.make_camera(257 * 16, 16)
    gy = 16 if gx == 16 else 1
    n1, n2, n4 = 1500, 400, (200 if gy > 1 else 0)
    px, py, tt = _mixed(rng, gx, gy, n1, n2, n4)
    px[0], py[0] = centres(gx - 1, gy - 1)   # the last tile is not empty
    tt[0] = 1
    kinds = {k: int((tt == k).sum()) for k in (1, 2, 4)}
    return make_case(name, cam, px, py, uniform_bits(rng, len(px)), dict(kinds=kinds, R=int(tt.sum()), culled=0, tiles=gx * gy), seed=gx)


def _case_D4(name):
    """524 304 x 17: tile row 1 is one pixel high.  Radius-3 Gaussians (scale 1e-6 at this focal length) at py = 7.5 touch row 0 only, at
    py = 15.5 both rows, at py = 19.5 (below the image) row 1 only."""
    rng = np.random.default_rng(4)
    cam = gsr_scene.make_camera(D4_W, D4_H, fovx=2.6)
    gx = (D4_W + 15) // 16
    n = 2900
    col = rng.integers(0, gx, n)
    row_kind = rng.integers(0, 3, n)            # 0: row 0, 1: both, 2: row 1
    on_seam = rng.random(n) < 0.3
    col[on_seam] = np.maximum(col[on_seam], 1)
    # the last two tile ids, 65 536 = (32 767, 1) and 65 537 = (32 768, 1): 30 Gaussians in each alone, 40 across both rows there
    extra_col = np.concatenate([np.full(30, gx - 2), np.full(30, gx - 1), np.full(20, gx - 2), np.full(20, gx - 1)])
    extra_kind = np.concatenate([np.full(60, 2), np.full(40, 1)])
    col = np.concatenate([col, extra_col]); row_kind = np.concatenate([row_kind, extra_kind]); on_seam = np.concatenate([on_seam, np.zeros(100, bool)])
    px = np.where(on_seam, 16.0 * col - 0.5, 16.0 * col + 7.5)
    py = np.array([7.5, 15.5, 19.5])[row_kind]
    w, h = np.where(on_seam, 2, 1), np.where(row_kind == 1, 2, 1)
    p = rng.permutation(len(px))
    shapes = np.stack([w, h], 1)[p]
    exp = dict(shapes=shapes, R=int((w * h).sum()), culled=0, tiles=65538, straddle_min=20, last_tiles_min=20)
    return make_case(name, cam, px[p], py[p], uniform_bits(rng, len(px)), exp, scales=1e-6, seed=4)


E_NAMES = [f"E_{P}" for P in (4096 * 1024, 4096 * 1024 + 1)]
E_BLOCK, E_CHUNK = 1024, 64          # TB_BLOCK (segments per workgroup of both column-pair passes), GSR_SORT_CHUNK (blocks per chunk)
E_SORT_SMALL_N = 4 << 20             # GSR_SORT_SMALL_N: the radix passes take 4 keys per thread up to here, 16 beyond


def blocks_and_chunks(col_pairs):
    """Workgroups ("blocks") and chunks of the two column-pair passes for these pairs per tile column: pass 1 cuts all pairs into blocks
    of 1 024, pass 2's blocks are column-aligned (csrc/tilebin.hip tb_col_blocks, tb_row_map).  Three levels of offset tables iff
    chunks > 64 (csrc/gsr_radix_walk.h)."""
    n = np.asarray(col_pairs, np.int64)
    b1, b2 = -(-int(n.sum()) // E_BLOCK), int((-(-n // E_BLOCK)).sum())
    return dict(pass1=(b1, -(-b1 // E_CHUNK)), pass2=(b2, -(-b2 // E_CHUNK)))


def _case_E(name):
    """Single-tile Gaussians on 256 x 256, exactly 256 Ki in each of the 16 tile columns -- so that pass 2, whose workgroups are
    column-aligned, has 4 096 blocks = 64 chunks like pass 1 -- and, for P + 1, one more in column 5: 4 097 blocks = 65 chunks in both."""
    P = int(name[2:])
    rng = np.random.default_rng(P & 0xFFFF)
    cam = gsr_scene.make_camera(256, 256)
    cols = np.repeat(np.arange(16), 4096 * 1024 // 16)
    if P > len(cols):
        cols = np.concatenate([cols, [5]])
    cols = rng.permutation(cols)
    px, py = centres(cols, rng.integers(0, 16, P))
    levels = (4096, 64) if P == 4096 * 1024 else (4097, 65)
    exp = dict(kinds={1: P, 2: 0, 4: 0}, pairs=P, R=P, culled=0, col_pairs=np.bincount(cols, minlength=16), pass1=levels, pass2=levels)
    return make_case(name, cam, px, py, uniform_bits(rng, P), exp, seed=1)


F_NAMES = ["F_9216_tiles", "F_9217_tiles"]
F_SIZES = {"F_9216_tiles": (1536, 1536), "F_9217_tiles": (208, 11344)}


def _case_F(name):
    """3 000 random Gaussians (gsr_scene.make_scene) on an image of 9 216 / 9 217 tiles: the tile-order kernel keeps the bins of the first
    9 216 tiles in registers."""
    W, H = F_SIZES[name]
    scene = gsr_scene.make_scene(3000, -3.0, sh_degree=0, seed=W)
    g = torch.Generator().manual_seed(H)
    colors = torch.rand(3000, 3, generator=g)
    cam = gsr_scene.make_camera(W, H)
    T = ((W + 15) // 16) * ((H + 15) // 16)
    return Case(name, scene, colors, cam, None, dict(P=3000, tiles=T))


_BUILDERS = {"A": _case_A, "B": _case_B, "C1": _case_C1, "C2": _case_C2, "C3": _case_C3, "C4": _case_C4, "C5": _case_C5, "D1": _case_D1,
             "D2": _case_D2, "D3": _case_D3, "D4": _case_D4, "E": _case_E, "F": _case_F}
C_NAMES = C1_NAMES + C2_NAMES + C3_NAMES + C4_NAMES + C5_NAMES
D_SMALL_NAMES = D1_NAMES + D2_NAMES + D3_NAMES
ALL_NAMES = A_NAMES + B_NAMES + C_NAMES + D_SMALL_NAMES + [D4_NAME] + E_NAMES + F_NAMES


@functools.lru_cache(maxsize=4)
def case(name):
    return _BUILDERS[name.split("_")[0]](name)


@functools.lru_cache(maxsize=4)
def oracle_state(name):
    """The C oracle's forward of a case (shared by the tests that need it; do not modify)."""
    import util
    c = case(name)
    return util.oracle_forward(c.scene, c.cam, 0, colors_precomp=c.colors, use_sh=False)
