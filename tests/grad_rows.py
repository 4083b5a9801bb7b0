"""Per-row gradient bounds of the backward blend (oracle.blend_backward_budget) and the small scenes whose rows are small on
purpose.  Shared by tests/test_grad_rows_cpu.py, tests/test_grad_rows_gpu.py and the per-row level of
tests/test_parity_gpu.py check_grads.  The derivation of the bound stands in tests/test_grad_rows_gpu.py."""
import numpy as np
import torch

import gsr_scene
from oracle import oracle

TENSORS = oracle.BLEND_TENSORS
CAP = 1e-3          # "the bound is not vacuous": E <= CAP |S| ...
CAP_SHARE = 0.90    # ... on this share of the rows with S != 0
SLOT_COOP, SLOT_ROUND = 30, 6   # csrc/gaussian_backward.hip GSR_SLOT_COOP, GSR_SLOT_ROUND
RUN_LENGTHS = (1, 2, 5, 6, 7, 12, 13, 29, 30, 31, 32, 62, 64, 65, 128)


def components(g):
    """The components the blend defines, out of gradient tensors laid out as the rasterizer returns them: dL_dmeans2D (P,3) ->
    (P,2), dL_dconic (P,2,2) or (P,4) -> (P,3) = (.x, .y, .w), dL_dopacity (P,1), dL_dcolors (P,3)."""
    P = np.asarray(g["dL_dopacity"]).reshape(-1).shape[0]
    return dict(dL_dmeans2D=np.asarray(g["dL_dmeans2D"]).reshape(P, -1)[:, :2],
                dL_dconic=np.asarray(g["dL_dconic"]).reshape(P, 4)[:, [0, 1, 3]],
                dL_dopacity=np.asarray(g["dL_dopacity"]).reshape(P, 1),
                dL_dcolors=np.asarray(g["dL_dcolors"]).reshape(P, 3))


def row_ratios(g, bud):
    """-> {tensor: (largest err / E over the rows with terms, rows and components outside E, rows without terms that do not
    hold +0 bits)} for fp32 blend sums g (any layout `components` takes) against a budget of oracle.blend_backward_budget."""
    c = components(g)
    has = bud["n"] > 0
    out = {}
    for k in TENSORS:
        got = c[k]
        err = np.abs(got.astype(np.float64) - bud["S"][k])
        E = bud["E"][k]
        ratio = np.where(E > 0, err / np.where(E > 0, E, 1.0), np.where(err > 0, np.inf, 0.0))
        empty = np.ascontiguousarray(got[~has], dtype=np.float32).view(np.uint32)
        out[k] = (float(ratio[has].max()) if has.any() else 0.0, np.argwhere(err > E), np.flatnonzero(empty.any(axis=1)))
    return out


def format_ratios(r):
    return "\n".join(f"rows:{k:22s} largest err / E {r[k][0]:.3f}" for k in TENSORS)


def rows_failures(g, bud):
    """The rows and components of g outside the per-row bound, as text (empty: the check passes)."""
    r = row_ratios(g, bud)
    c = components(g)
    bad = []
    for k in TENSORS:
        _, outside, nonzero = r[k]
        for i, j in outside[:5]:
            bad.append(f"{k}[{i},{j}] = {c[k][i, j]!r}, float64 {bud['S'][k][i, j]!r}, E {bud['E'][k][i, j]:.3e}, n {bud['n'][i]}")
        if len(outside) > 5:
            bad.append(f"{k}: {len(outside)} rows and components outside E")
        if len(nonzero):
            bad.append(f"{k}: rows without terms that are not +0: {nonzero[:5]}")
    return r, bad


def cap_shares(bud):
    """-> {tensor: the share of rows with S != 0 on which E <= CAP |S| holds}.  A row of several components is taken as the
    vector training takes it for (densification thresholds the norm of a dL/dmean2D row): max_c E <= CAP max_c |S|, so a
    component that vanishes by symmetry (the conic's b under a round splat) does not speak for its row."""
    out = {}
    for k in TENSORS:
        S, E = np.abs(bud["S"][k]).max(axis=1), bud["E"][k].max(axis=1)
        rows = S != 0
        out[k] = float((E[rows] <= CAP * S[rows]).mean()) if rows.any() else 1.0
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# scenes.  Each is a few hundred Gaussians; colours come from degree-0 SH so every caller can use the usual leaves.

def _scene(px, py, z, radius, opac, W, H, fovx, seed):
    """Isotropic Gaussians whose projections have the pixel centres (px, py) at view depth z (camera at (0, 0, -4) looking down
    +z) and the integer screen radius `radius`.  An isotropic Gaussian of scale s projects to the covariance
    (f s / z)^2 (I + t t^T) + 0.3 I with t = (x / z, y / z) clamped to 1.3 tan(fov / 2) (forward.cu:84-140), so its largest
    eigenvalue is (f s / z)^2 (1 + |t|^2) + 0.3 and the radius is ceil(3 sqrt(that)): s is chosen to put 3 sqrt(.) at radius - 0.5."""
    P = len(px)
    g = torch.Generator().manual_seed(seed)
    tx = np.tan(fovx * 0.5)
    ty = tx * H / W
    focal = W / (2.0 * tx)
    # pix = ((ndc + 1) S - 1) / 2 with ndc = x / (z tan)
    x = ((2.0 * px + 1.0) / W - 1.0) * tx * z
    y = ((2.0 * py + 1.0) / H - 1.0) * ty * z
    t2 = np.clip(x / z, -1.3 * tx, 1.3 * tx) ** 2 + np.clip(y / z, -1.3 * ty, 1.3 * ty) ** 2
    lam = ((radius - 0.5) / 3.0) ** 2 - 0.3
    s = np.sqrt(lam / (1.0 + t2)) * z / focal
    means = torch.from_numpy(np.stack([x, y, z - 4.0], axis=-1)).float()
    scales = torch.from_numpy(s).float().reshape(P, 1).repeat(1, 3)
    rot = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(P, 1)
    shs = torch.randn(P, 1, 3, generator=g)
    return gsr_scene.Scene(means.contiguous(), scales.contiguous(), rot.contiguous(), torch.from_numpy(opac).float().reshape(P, 1).contiguous(),
                           shs.contiguous(), torch.tensor([0.1, 0.2, 0.3]))


SLOT_W, SLOT_H, SLOT_FOVX = 512, 128, 1.0
# tiles_touched = w x h tiles of the 32 x 8 grid
SLOT_RECTS = {1: (1, 1), 2: (2, 1), 5: (5, 1), 6: (3, 2), 7: (7, 1), 12: (4, 3), 13: (13, 1), 29: (29, 1), 30: (6, 5), 31: (31, 1),
              32: (8, 4), 62: (31, 2), 64: (8, 8), 65: (13, 5), 128: (16, 8)}
SLOT_P = 64 * 6 + 37   # the last Gaussian sits in mid-wave


def slot_runs_scene():
    """Every run length of RUN_LENGTHS at every residue of slot_base mod 4 (slot_base = the exclusive prefix of tiles_touched in
    index order): for each length and each residue a splat of that many tiles, preceded by as many one-tile fillers as move
    the prefix to the residue; then fillers up to SLOT_P Gaussians.
    A splat of w x h tiles, w >= h: radius r = 8 w - 6 (4 for one tile) around cx = 16 x0 + 8 w - 0.5 gives the columns
    floor((cx - r) / 16) = x0 ... floor((cx + r + 15) / 16) - 1 = x0 + w - 1 (auxiliary.h:48-58); where h < w the centre
    lies at cy = 16 h - 8 - r, near or above the top border, which cuts the rectangle to the rows 0 ... h - 1.  The circle of a
    large splat misses the corner tiles of its rectangle: the trim leaves them out, and without the trim no pixel of them is hit.
    -> (scene, camera, {(length, residue): Gaussian index})"""
    W, H, fovx = SLOT_W, SLOT_H, SLOT_FOVX
    rng = np.random.RandomState(7)
    px, py, rad, opac = [], [], [], []
    runs = {}
    total = 0

    def filler():
        nonlocal total
        tx, ty = rng.randint(0, W // 16), rng.randint(0, H // 16)
        px.append(16 * tx + 4.5 + 7 * rng.rand()); py.append(16 * ty + 4.5 + 7 * rng.rand()); rad.append(4); opac.append(0.3 + 0.4 * rng.rand())
        total += 1

    for L in RUN_LENGTHS:
        w, h = SLOT_RECTS[L]
        for res in range(4):
            while total % 4 != res:
                filler()
            r = max(8 * w - 6, 4)
            x0 = rng.randint(0, W // 16 - w + 1)
            cx = 16 * x0 + 8 * w - 0.5
            cy = 16 * rng.randint(0, H // 16) + 7.5 if h == w == 1 else (8 * w - 0.5 if h == w else 16 * h - 8 - r)
            px.append(cx); py.append(cy); rad.append(r)
            # a centre far above the image reaches it only with the tail of a strong Gaussian; one on the image stays faint so
            # that T stays well above 1e-4 behind the stack of large splats
            opac.append(0.9 if cy < -r / 2 else 0.05 + 0.1 * rng.rand())
            runs[(L, res)] = len(px) - 1
            total += L
    assert len(px) <= SLOT_P
    while len(px) < SLOT_P:
        filler()
    P = len(px)
    z = 4.0 + rng.rand(P)
    scene = _scene(np.array(px), np.array(py), z, np.array(rad, dtype=np.float64), np.array(opac), W, H, fovx, seed=70)
    return scene, gsr_scene.make_camera(W, H, fovx=fovx), runs


def assert_slot_runs(tiles_touched, runs):
    """the slot-run fixture is what it claims, from the oracle's (or the kernels') tiles_touched"""
    tt = np.asarray(tiles_touched).astype(np.int64)
    base = np.cumsum(tt) - tt
    assert set(runs) == {(L, res) for L in RUN_LENGTHS for res in range(4)}
    for (L, res), i in runs.items():
        assert tt[i] == L and base[i] % 4 == res, f"Gaussian {i}: {tt[i]} tiles at slot_base {base[i]}, wanted {L} at residue {res}"
    others = np.setdiff1d(np.arange(len(tt)), list(runs.values()))
    assert (tt[others] == 1).all(), "a filler that does not touch exactly one tile"


def assert_deep_tile(o, bud):
    """the deep-tile fixture is what it claims: every pixel's walk ends on n_contrib inside the list (T passed 1e-4), and the
    rows with terms span more than four decades"""
    assert o["num_rendered"] == o["P"] and (o["W"], o["H"]) == (16, 16)
    assert 0 < o["n_contrib"].min() and o["n_contrib"].max() < o["num_rendered"], "a walk that ends on the list"
    m = np.abs(bud["S"]["dL_dopacity"][:, 0])
    m = m[bud["n"] > 0]
    assert m.min() > 0 and m.max() / m.min() > 1e4, m.max() / m.min()
    assert (bud["n"] == 0).any(), "no Gaussian behind the last contributor"


def deep_tile_scene(P=200):
    """One 16 x 16 tile, P Gaussians of opacity 0.3 ... 0.6, each wide enough to cover it: T passes 1e-4 inside the list at every
    pixel, so every walk ends on n_contrib and the rows behind carry next to nothing."""
    rng = np.random.RandomState(11)
    W = H = 16
    fovx = 0.15
    z = 3.5 + rng.rand(P)
    rad = rng.randint(11, 22, size=P).astype(np.float64)   # sigma 3.5 ... 7 pixels
    scene = _scene(2.0 + 12.0 * rng.rand(P), 2.0 + 12.0 * rng.rand(P), z, rad, 0.3 + 0.3 * rng.rand(P), W, H, fovx, seed=71)
    return scene, gsr_scene.make_camera(W, H, fovx=fovx)


HEAVY_P, HEAVY_W, HEAVY_H = 3_200, 144, 144


def heavy_scene():
    """The recipe of tests/test_backward_flush_gpu.py _heavy_scene (a dense, low-opacity blob in front of a sparse cloud), cut
    down: on 144 x 144 pixels the blob (2 400 of the 3 200 Gaussians) falls on the centre tile, a list of more than 4 x 512
    instances; 9 x 9 tiles, because the dispatch cuts no walk and splits no tile on an image of fewer than 64
    (csrc/binning.hip gsr_tile_order_max_segments)."""
    P, W, H, D = HEAVY_P, HEAVY_W, HEAVY_H, 1
    scene = gsr_scene.make_scene(P, -3.6, sh_degree=D, seed=21)
    g = torch.Generator().manual_seed(22)
    nb = P * 3 // 4
    means = scene.means3D.clone()
    means[:nb] = torch.randn(nb, 3, generator=g) * torch.tensor([0.1, 0.07, 0.3])
    opac = scene.opacities.clone()
    opac[:nb] = torch.sigmoid(torch.randn(nb, 1, generator=g) - 3.5)
    return scene._replace(means3D=means.contiguous(), opacities=opac.contiguous()), gsr_scene.make_camera(W, H), D


WAVES = (8.0, 16.0, 32.0, 64.0, 128.0)
CASE_RAMP = 16.0   # e-folding length in pixels of the ramp the parity CASES are measured under (test_grad_rows_cpu.py)


def smooth_dpix(o, cam, seed=1, ramp=0.0):
    """An upstream gradient without white noise, zero on the oracle's fragile pixels like util.fragile_free_dpix: per channel
    1 + five plane waves of wavelength 8 ... 128 pixels (amplitude 0.18 each, seeded direction and phase).  It stays positive, so
    a row's terms differ in sign only through the scene (colour against the colour behind, the side of the mean a pixel lies
    on), and it has a slope at every splat size, so dL/dmean2D does not vanish by symmetry.  ramp: times exp((x + y) / ramp),
    normalised to 1 at the centre -- the same relative slope under every splat; a row's bound scales with the row, so the
    image-wide range costs nothing."""
    H, W = cam.image_height, cam.image_width
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    d = np.ones((3, H, W))
    for ch in range(3):
        for lam in WAVES:
            th, ph = rng.rand() * 2.0 * np.pi, rng.rand() * 2.0 * np.pi
            d[ch] += 0.18 * np.sin(2.0 * np.pi * (x * np.cos(th) + y * np.sin(th)) / lam + ph)
    if ramp:
        d *= np.exp((x + y - 0.5 * (W + H)) / ramp)
    ok = (o["fragile"] == 0).reshape(H, W)
    return torch.from_numpy((d * ok).astype(np.float32))
