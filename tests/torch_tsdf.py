"""Float64 reference of TSDF fusion and marching tetrahedra (include/gsr_tsdf.h, fused_tsdf.py) in numpy, restated from the header's
rule and sharing no table with the kernels: the triangles of a tetrahedron come from the generic rule (one corner apart: a triangle;
two inside: a quadrilateral split by the header's sentence) and their orientation from a cross product against the gradient of the
tetrahedron's linear interpolant.  Also the test scenes and fields, so that the CPU tests that qualify them and the GPU tests that use
them look at the same numbers, and the topology checks both apply.  mesh_ref is the rule as three loops; mesh_ref_fast is the same
rule in array operations, for volumes large enough to reach the seams of the plan's scan, with its table filled in from tet_triangles."""
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
# the integration cases of tests/test_tsdf_gpu.py: a lone lane, a few lanes, a full wave and one over it, one brick of 8 x 8 x 4 and one over
# it in each axis, several workgroups with a remainder
GRIDS = ((1, 1, 1), (5, 3, 2), (64, 1, 1), (65, 3, 3), (8, 8, 4), (9, 8, 5), (33, 17, 9))
CAMERAS = (1, 3, 5)
IMAGES = ((37, 23), (64, 16))   # W x H
SDF_TRUNC, DEPTH_TRUNC = 0.25, 4.75
# the extraction cases: the two grids of the CPU test, the smallest grids, and the integration grids that have cells
MESH_GRIDS = ((12, 11, 10), (17, 9, 8), (2, 2, 2), (3, 2, 2), (5, 3, 2), (65, 3, 3), (8, 8, 4), (9, 8, 5), (33, 17, 9))
KINDS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1))   # the edge kinds a node owns, in the header's order
AXIS_ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))        # tetrahedra 0..5: xyz, xzy, yxz, yzx, zxy, zyx


# ---- cameras and scenes ----
def look_at(pos, target, W, H, f, up=(0.0, 1.0, 0.0)):
    """-> one packed record (20,) float32: a camera at `pos` looking at `target`, focal f, centred"""
    pos, target, up = (np.asarray(v, np.float64) for v in (pos, target, up))
    zax = (target - pos) / np.linalg.norm(target - pos)
    xax = np.cross(up, zax)
    xax /= np.linalg.norm(xax)
    yax = np.cross(zax, xax)
    R = np.stack([xax, yax, zax])
    rec = np.zeros(20, np.float32)
    rec[0:9] = R.reshape(-1)
    rec[9:12] = -R @ pos
    rec[12:18] = (f, f * 1.07, 0.5 * W + 0.3, 0.5 * H - 0.2, W, H)
    return rec


def grid_of(dims):
    """the integration grid of `dims`: inside [-1, 1]^3 around the origin -> (origin (3,) float32, voxel_size float32)"""
    vs = np.float32(2.0 / max(max(dims) - 1, 4))
    origin = np.array([-0.5 * (n - 1) * float(vs) for n in dims], np.float32)
    return origin, vs


def integration_scene(dims, C, image):
    """-> a namespace of float32 arrays: origin, voxel_size, rec (C,20), depth (C,H,W), color (C,3,H,W), weight (C,H,W), and the planes'
    previous contents wsum0, dsum0 (NZ,NY,NX), csum0 (3,NZ,NY,NX).  Camera 0 stands in front of the grid; camera 1 beside it, looking
    past it; camera 2 with its back to it; 3 and 4 in front again from other sides.  The depth maps are a wavy surface through the grid
    (4 + 0.9 sin(0.9 u + c) cos(0.45 v - c / 2 + 2.1): in front of some nodes by more than the truncation, behind others) with zeros,
    negatives, NaN, +inf and values beyond DEPTH_TRUNC sprinkled in; the weights have zeros, negatives, NaN and +inf."""
    W, H = image
    rng = np.random.default_rng(1000 * (dims[0] * 10000 + dims[1] * 100 + dims[2]) + 10 * C + W)
    f = 0.5 * W / 0.33
    places = [((0.3, 0.4, -4.0), (0, 0, 0)), ((4.0, 0.2, 0.5), (4.0, 0.0, 5.0)), ((0.0, 0.5, 4.0), (0.0, 1.0, 9.0)), ((-3.2, 0.3, -2.4), (0.1, 0, 0)),
              ((2.6, -1.0, -3.0), (0, 0.1, 0))]
    rec = np.stack([look_at(p, t, W, H, f) for p, t in places[:C]])
    uu, vv = np.meshgrid(np.arange(W), np.arange(H))
    depth = np.stack([4.0 + 0.9 * np.sin(0.9 * uu + c) * np.cos(0.45 * vv - 0.5 * c + 2.1) for c in range(C)]).astype(np.float32)
    r = rng.random(depth.shape)
    for lo, hi, val in ((0.00, 0.03, 0.0), (0.03, 0.05, np.nan), (0.05, 0.07, np.inf), (0.07, 0.10, 5.5), (0.10, 0.11, -1.0)):
        depth[(r >= lo) & (r < hi)] = val
    weight = (0.5 + 1.5 * rng.random(depth.shape)).astype(np.float32)
    r = rng.random(depth.shape)
    weight[r < 0.2] = 0.0
    weight[(r >= 0.2) & (r < 0.21)] = np.nan
    weight[(r >= 0.21) & (r < 0.22)] = np.inf
    weight[(r >= 0.22) & (r < 0.23)] = -1.0
    color = rng.random((C, 3, H, W)).astype(np.float32)
    origin, vs = grid_of(dims)
    shape = dims[::-1]
    return SimpleNamespace(dims=dims, origin=origin, voxel_size=vs, rec=rec, depth=depth, color=color, weight=weight, W=W, H=H,
                           wsum0=(0.25 + rng.random(shape)).astype(np.float32), dsum0=(rng.random(shape) - 0.5).astype(np.float32),
                           csum0=rng.random((3,) + shape).astype(np.float32))


def node_positions(dims, origin, voxel_size):
    """-> (nodes, 3) float64 in node order (x fastest)"""
    k, j, i = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    ijk = np.stack([i.reshape(-1), j.reshape(-1), k.reshape(-1)], axis=1).astype(np.float64)
    return np.asarray(origin, np.float64)[None, :] + ijk * float(voxel_size)


# ---- integration ----
def integrate_ref(dims, origin, voxel_size, rec, depth, color=None, weight=None, sdf_trunc=SDF_TRUNC, depth_trunc=DEPTH_TRUNC, wsum0=None,
                  dsum0=None, csum0=None):
    """The rule of gsr_tsdf.h in float64 from the float32 inputs -> a namespace, everything per node in node order:
    wsum, dsum (nodes,), csum (3, nodes): the sums; touched: some camera added to the node;
    ambiguous: some camera's decision lies within the float32 error of its own inputs (bands below);
    bound_w, bound_d, bound_c: the error the float32 sums may carry at an unambiguous node;
    skipped, cut, clamped: how many node-camera pairs were skipped (behind, beside the image, no valid depth or weight), cut at
    -sdf_trunc, and clamped to 1.

    Bands, from the operation count of the kernel's rule (u = 2^-24; S_j = sum_k |R_jk x_k| + |t_j|): a coordinate is one fma (u |x_k|), a
    camera-space component a chain of three more (3 u S_j): 4 u S_j, taken as E_j = 8 u S_j.
      p_z > 0                 |p_z| <= E_z
      floor(U), floor(V)      U = fma(p_x rcp(p_z), fx, cx): the errors of p_x and p_z carried through the quotient, the reciprocal
                              (2 u), the product (u) and the fma (u): E_U = fx / p_z (E_x + |p_x| / p_z E_z) + 4 u |fx p_x / p_z| + 2 u
                              (|U| + |cx|); open where U lies within E_U of an integer (any integer: it changes the pixel) in or next to
                              the image
      d <= depth_trunc        a comparison of two float32 inputs: exact, no band
      sdf >= -trunc, >= trunc sdf = d - p_z: E_s = E_z + 2 u (|d| + |p_z|); open where |sdf + trunc| or |sdf - trunc| <= E_s
    Sums: tsdf = min(1, sdf fp32(1 / trunc)) carries E_s / trunc + 3 u |tsdf| (the rounded reciprocal, the product); each of the C
    additions rounds a partial sum that is at most the sum of the moduli: (C + 1) u (|start| + sum |term|)."""
    C, H, W = depth.shape
    nodes = dims[0] * dims[1] * dims[2]
    x = node_positions(dims, origin, voxel_size)
    ax = np.abs(x)
    start = lambda t, shape: np.zeros(shape) if t is None else np.asarray(t, np.float64).reshape(shape)
    out = SimpleNamespace(wsum=start(wsum0, nodes), dsum=start(dsum0, nodes), csum=start(csum0, (3, nodes)), skipped=0, cut=0, clamped=0)
    mod_w, mod_d, mod_c = np.abs(out.wsum), np.abs(out.dsum), np.abs(out.csum)
    term_d = np.zeros(nodes)
    out.touched, out.ambiguous = np.zeros(nodes, bool), np.zeros(nodes, bool)
    trunc, inv = float(np.float32(sdf_trunc)), 1.0 / float(np.float32(sdf_trunc))
    for c in range(C):
        r = rec[c].astype(np.float64)
        R, t = r[:9].reshape(3, 3), r[9:12]
        fx, fy, cx, cy = r[12:16]
        p = x @ R.T + t
        E = 8 * U * (ax @ np.abs(R).T + np.abs(t))
        pz = p[:, 2]
        front = pz > 0
        amb = np.abs(pz) <= E[:, 2]
        pzs = np.where(front, pz, 1.0)
        qx, qy = fx * p[:, 0] / pzs, fy * p[:, 1] / pzs
        Uc, Vc = qx + cx, qy + cy
        EU = np.abs(fx) / pzs * (E[:, 0] + np.abs(p[:, 0]) / pzs * E[:, 2]) + 4 * U * np.abs(qx) + 2 * U * (np.abs(Uc) + abs(cx))
        EV = np.abs(fy) / pzs * (E[:, 1] + np.abs(p[:, 1]) / pzs * E[:, 2]) + 4 * U * np.abs(qy) + 2 * U * (np.abs(Vc) + abs(cy))
        near = (Uc > -1) & (Uc < W + 1) & (Vc > -1) & (Vc < H + 1)
        amb |= front & near & ((np.abs(Uc - np.rint(Uc)) <= EU) | (np.abs(Vc - np.rint(Vc)) <= EV))
        inside = front & (Uc >= 0) & (Uc < W) & (Vc >= 0) & (Vc < H)
        pu, pv = np.where(inside, np.floor(Uc), 0).astype(np.int64), np.where(inside, np.floor(Vc), 0).astype(np.int64)
        d = depth[c, pv, pu].astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok = inside & np.isfinite(d) & (d > 0) & (d <= float(np.float32(depth_trunc)))
            ds = np.where(ok, d, 0.0)
            sdf = ds - pz
            Es = E[:, 2] + 2 * U * (np.abs(ds) + np.abs(pz))
            amb |= ok & ((np.abs(sdf + trunc) <= Es) | (np.abs(sdf - trunc) <= Es))
            kept = ok & (sdf >= -trunc)
            tsdf = np.minimum(1.0, sdf * inv)
            w = weight[c, pv, pu].astype(np.float64) if weight is not None else np.ones(nodes)
            add = kept & np.isfinite(w) & (w > 0)
        w = np.where(add, w, 0.0)
        tsdf = np.where(add, tsdf, 0.0)
        out.skipped += int((~ok).sum() + (kept & ~add).sum())
        out.cut += int((ok & ~kept).sum())
        out.clamped += int((add & (sdf * inv >= 1.0)).sum())
        out.wsum = out.wsum + w
        out.dsum = out.dsum + w * tsdf
        mod_w = mod_w + w
        mod_d = mod_d + w * np.abs(tsdf)
        term_d = term_d + w * (Es * inv + 3 * U * np.abs(tsdf))
        if color is not None:
            rgb = color[c][:, pv, pu].astype(np.float64)
            out.csum = out.csum + w[None, :] * np.where(add[None, :], rgb, 0.0)
            mod_c = mod_c + w[None, :] * np.abs(np.where(add[None, :], rgb, 0.0))
        out.touched |= add
        out.ambiguous |= amb
    out.bound_w = (C + 1) * U * mod_w
    out.bound_d = term_d + (C + 1) * U * mod_d
    out.bound_c = (C + 1) * U * mod_c
    return out


# ---- marching tetrahedra ----
def _corner(path, axes):
    """the cell corner (dx, dy, dz) after the first `path` steps of the axis order"""
    c = [0, 0, 0]
    for a in axes[:path]:
        c[a] = 1
    return tuple(c)


def _orientation(corners, inside, tri):
    """+1 where the triangle over the edges `tri` (pairs of path corners), with its vertices at the edges' midpoints, looks along the
    gradient of the linear interpolant of the sign field (-1 inside, +1 outside), else -1.  The answer depends on the signs only."""
    P = np.array(corners, np.float64)
    s = np.array([-1.0 if i else 1.0 for i in inside])
    g = np.linalg.solve(P[1:] - P[0], s[1:] - s[0])
    m = [0.5 * (P[a] + P[b]) for a, b in tri]
    n = np.cross(m[1] - m[0], m[2] - m[0])
    dot = float(n @ g)
    assert abs(dot) > 1e-9
    return 1 if dot > 0 else -1


def tet_triangles(corners, inside):
    """The generic rule -> the triangles of one tetrahedron as triples of edges (lo, hi) of path corners, oriented counter-clockwise seen
    from the positive side."""
    ins = [l for l in range(4) if inside[l]]
    outs = [l for l in range(4) if not inside[l]]
    edge = lambda a, b: (min(a, b), max(a, b))
    if len(ins) in (0, 4):
        return []
    if len(ins) in (1, 3):
        a = (ins if len(ins) == 1 else outs)[0]
        b, c, d = [l for l in range(4) if l != a]
        tris = [[edge(a, b), edge(a, c), edge(a, d)]]
    else:
        (a, b), (c, d) = ins, outs
        ac, ad, bd, bc = edge(a, c), edge(a, d), edge(b, d), edge(b, c)
        tris = [[ac, ad, bd], [ac, bd, bc]]   # the diagonal ac-bd; the first triangle holds ad
    return [t if _orientation(corners, inside, t) > 0 else [t[0], t[2], t[1]] for t in tris]


def mesh_ref(wsum, dsum, origin, voxel_size, min_weight=1.0, csum=None):
    """wsum, dsum (NZ,NY,NX) float32, csum (3,NZ,NY,NX) or None -> a namespace: vertices (V,3) float64, colors (V,3) float64 or None,
    faces (F,3) int64, and per vertex: lower (V,3) and upper (V,3) the positions of its edge's nodes, v0, v1 (V,) their values, t (V,),
    c0, c1 (V,3) their colours, node, kind (V,) the lower node's index and the rank of the edge's kind; per face: cell (the index of the
    cell's node), tet (0..5) and case (sum of 2^l over the inside path corners l) of the tetrahedron that emits it."""
    NZ, NY, NX = wsum.shape
    w, d = wsum.astype(np.float64), dsum.astype(np.float64)
    with np.errstate(invalid="ignore"):
        valid = w >= float(np.float32(min_weight))
    val = np.where(valid, d / np.where(valid, w, 1.0), np.nan)
    inside = valid & (val < 0)
    col = None if csum is None else np.where(valid[None], csum.astype(np.float64) / np.where(valid, w, 1.0)[None], np.nan)
    org, vs = np.asarray(origin, np.float64), float(voxel_size)
    ids, rows = {}, []
    for k in range(NZ):
        for j in range(NY):
            for i in range(NX):
                if not valid[k, j, i]:
                    continue
                for kind, (dx, dy, dz) in enumerate(KINDS):
                    i1, j1, k1 = i + dx, j + dy, k + dz
                    if i1 >= NX or j1 >= NY or k1 >= NZ or not valid[k1, j1, i1] or inside[k, j, i] == inside[k1, j1, i1]:
                        continue
                    v0, v1 = val[k, j, i], val[k1, j1, i1]
                    t = v0 / (v0 - v1)
                    lo, up = org + np.array([i, j, k]) * vs, org + np.array([i1, j1, k1]) * vs
                    ids[(i, j, k, kind)] = len(rows)
                    rows.append((lo + t * (up - lo), lo, up, v0, v1, t, None if col is None else col[:, k, j, i], None if col is None else col[:, k1, j1, i1],
                                 i + NX * (j + NY * k), kind))
    faces, emitters = [], []
    for k in range(NZ - 1):
        for j in range(NY - 1):
            for i in range(NX - 1):
                for axes in AXIS_ORDERS:
                    corners = [_corner(s, axes) for s in range(4)]
                    at = [(k + c[2], j + c[1], i + c[0]) for c in corners]
                    if not all(valid[q] for q in at):
                        continue
                    for tri in tet_triangles(corners, [bool(inside[q]) for q in at]):
                        emitters.append((i + NX * (j + NY * k), AXIS_ORDERS.index(axes), sum(int(inside[q]) << l for l, q in enumerate(at))))
                        face = []
                        for lo, hi in tri:
                            cl, ch = corners[lo], corners[hi]
                            kind = KINDS.index((ch[0] - cl[0], ch[1] - cl[1], ch[2] - cl[2]))
                            face.append(ids[(i + cl[0], j + cl[1], k + cl[2], kind)])
                        faces.append(face)
    V = len(rows)
    col3 = lambda n: np.array([r[n] for r in rows], np.float64).reshape(V, 3)
    out = SimpleNamespace(vertices=col3(0), lower=col3(1), upper=col3(2), v0=np.array([r[3] for r in rows]), v1=np.array([r[4] for r in rows]),
                          t=np.array([r[5] for r in rows]), faces=np.array(faces, np.int64).reshape(-1, 3), colors=None,
                          node=np.array([r[8] for r in rows], np.int64), kind=np.array([r[9] for r in rows], np.int64))
    out.cell, out.tet, out.case = (np.array([e[n] for e in emitters], np.int64) for n in range(3))
    if col is not None:
        out.c0, out.c1 = col3(6), col3(7)
        out.colors = out.c0 + out.t[:, None] * (out.c1 - out.c0)
    return out


_rule = {}


def _rule_tables():
    """The generic rule laid out for array indexing, derived here from tet_triangles (and so from the cross product of _orientation),
    never typed in -> count (6, 16): the triangles of tetrahedron T in case m; lo (6, 16, 2, 3, 3): the cell corner (dx, dy, dz) that
    owns the edge of vertex s of triangle r; kind (6, 16, 2, 3): that edge's rank in KINDS."""
    if not _rule:
        count, lo, kind = np.zeros((6, 16), np.int64), np.zeros((6, 16, 2, 3, 3), np.int64), np.zeros((6, 16, 2, 3), np.int64)
        for T, axes in enumerate(AXIS_ORDERS):
            corners = [_corner(s, axes) for s in range(4)]
            for m in range(16):
                tris = tet_triangles(corners, [bool(m >> l & 1) for l in range(4)])
                count[T, m] = len(tris)
                for r, tri in enumerate(tris):
                    for s, (a, b) in enumerate(tri):
                        lo[T, m, r, s] = corners[a]
                        kind[T, m, r, s] = KINDS.index(tuple(corners[b][x] - corners[a][x] for x in range(3)))
        _rule.update(count=count, lo=lo, kind=kind)
    return _rule["count"], _rule["lo"], _rule["kind"]


def tet_census(wsum, min_weight, dsum):
    """Every tetrahedron of every cell, in arrays -> a namespace over the cells in cell index order (x fastest, cells only: NX - 1 by
    NY - 1 by NZ - 1): cell (cells,) the index of the cell's node, whole (cells, 6): all four corners valid, case (cells, 6): the sum of
    2^l over the path corners l that are valid and inside, crossed (cells, 6): some edge of the tetrahedron has two valid ends on
    different sides (it holds a vertex, whether or not the tetrahedron emits)."""
    NZ, NY, NX = wsum.shape
    with np.errstate(invalid="ignore"):
        valid = wsum.astype(np.float64) >= float(np.float32(min_weight))
    inside = valid & (dsum.astype(np.float64) / np.where(valid, wsum.astype(np.float64), 1.0) < 0)
    k, j, i = (a.reshape(-1) for a in np.meshgrid(np.arange(NZ - 1), np.arange(NY - 1), np.arange(NX - 1), indexing="ij"))
    cells = len(i)
    whole, case, crossed = np.ones((cells, 6), bool), np.zeros((cells, 6), np.int64), np.zeros((cells, 6), bool)
    for T, axes in enumerate(AXIS_ORDERS):
        at = [(k + c[2], j + c[1], i + c[0]) for c in (_corner(s, axes) for s in range(4))]
        for l in range(4):
            whole[:, T] &= valid[at[l]]
            case[:, T] |= inside[at[l]].astype(np.int64) << l
            for l2 in range(l):
                crossed[:, T] |= valid[at[l]] & valid[at[l2]] & (inside[at[l]] != inside[at[l2]])
    return SimpleNamespace(cell=i + NX * (j + NY * k), whole=whole, case=case, crossed=crossed)


def mesh_ref_fast(wsum, dsum, origin, voxel_size, min_weight=1.0, csum=None):
    """mesh_ref in array operations, for grids its loops cannot serve: the same arguments, the same namespace, and in every float64 field
    the same formula applied to the same doubles in the same order, so the bits are mesh_ref's (tests/test_tsdf_cpu.py holds it to that).
    Order by construction: the crossings as a (nodes, 7) array read in row-major order are the vertices in (node, kind) order; the
    triangle slots as a (cells, 6, 2) array read in row-major order are the faces in (cell, tetrahedron, triangle) order.  The rule
    comes from _rule_tables, that is from tet_triangles."""
    NZ, NY, NX = wsum.shape
    nodes = NX * NY * NZ
    w, d = wsum.astype(np.float64), dsum.astype(np.float64)
    with np.errstate(invalid="ignore"):
        valid = w >= float(np.float32(min_weight))
    val = np.where(valid, d / np.where(valid, w, 1.0), np.nan)
    inside = valid & (val < 0)
    col = None if csum is None else np.where(valid[None], csum.astype(np.float64) / np.where(valid, w, 1.0)[None], np.nan)
    org, vs = np.asarray(origin, np.float64), float(voxel_size)
    # vertices: crossing[n, kind], and ids[n, kind] = how many crossings come before it
    crossing = np.zeros((NZ, NY, NX, 7), bool)
    for kind, (dx, dy, dz) in enumerate(KINDS):
        low, up = (slice(0, NZ - dz), slice(0, NY - dy), slice(0, NX - dx)), (slice(dz, NZ), slice(dy, NY), slice(dx, NX))
        crossing[low + (kind,)] = valid[low] & valid[up] & (inside[low] != inside[up])
    crossing = crossing.reshape(nodes, 7)
    ids = (np.cumsum(crossing.reshape(-1), dtype=np.int64).reshape(nodes, 7) - 1)
    ids[~crossing] = -1
    node, kind = np.nonzero(crossing)
    ijk = np.stack([node % NX, (node // NX) % NY, node // (NX * NY)], axis=1)
    ijk1 = ijk + np.array(KINDS, np.int64)[kind]
    at0, at1 = (ijk[:, 2], ijk[:, 1], ijk[:, 0]), (ijk1[:, 2], ijk1[:, 1], ijk1[:, 0])
    v0, v1 = val[at0], val[at1]
    t = v0 / (v0 - v1)
    lo, up = org[None, :] + ijk * vs, org[None, :] + ijk1 * vs
    out = SimpleNamespace(vertices=lo + t[:, None] * (up - lo), lower=lo, upper=up, v0=v0, v1=v1, t=t, colors=None, node=node.astype(np.int64),
                          kind=kind.astype(np.int64))
    if col is not None:
        out.c0, out.c1 = col[(slice(None),) + at0].T.copy(), col[(slice(None),) + at1].T.copy()
        out.colors = out.c0 + out.t[:, None] * (out.c1 - out.c0)
    # faces: the cells that emit at all, then every triangle slot of theirs
    count, lo_corner, edge_kind = _rule_tables()
    cen = tet_census(wsum, min_weight, dsum)
    case = np.where(cen.whole, cen.case, 0)
    live = (count[np.arange(6)[None, :], case] > 0).any(axis=1)
    cell, case = cen.cell[live], case[live]
    Tn = np.broadcast_to(np.arange(6)[None, :], case.shape)
    emits = np.arange(2)[None, None, :] < count[Tn, case][:, :, None]                      # (cells, 6, 2)
    c = lo_corner[Tn, case]                                                                # (cells, 6, 2, 3, 3)
    owner = cell[:, None, None, None] + c[..., 0] + NX * (c[..., 1] + NY * c[..., 2])      # (cells, 6, 2, 3)
    faces = ids[np.where(emits[..., None], owner, 0), edge_kind[Tn, case]][emits]
    assert bool((faces >= 0).all())   # every vertex a triangle names is a crossing
    out.faces = faces.reshape(-1, 3)
    which = np.nonzero(emits)
    out.cell, out.tet, out.case = cell[which[0]], which[1].astype(np.int64), case[which[0], which[1]]
    return out


def rotate_to_smallest(faces):
    """every triangle rotated so that it begins with its smallest index: the cyclic order, which is all the contract fixes"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    s = f.argmin(axis=1)
    return np.stack([f[np.arange(len(f)), (s + r) % 3] for r in range(3)], axis=1)


def topology(faces):
    """-> a namespace: components (list of face-index arrays), and per component: closed (every undirected edge in exactly two faces,
    once in each direction), euler = V - E + F over the vertices it uses.  `manifold`: no directed edge occurs twice anywhere."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    directed = {}
    for n, (a, b, c) in enumerate(f):
        for e in ((a, b), (b, c), (c, a)):
            directed.setdefault(e, []).append(n)
    manifold = all(len(v) == 1 for v in directed.values()) and all(a != b for a, b in directed)
    parent = list(range(len(f)))

    def find(n):
        while parent[n] != n:
            parent[n] = parent[parent[n]]
            n = parent[n]
        return n

    for (a, b), owners in directed.items():
        for other in directed.get((b, a), []):
            parent[find(owners[0])] = find(other)
    groups = {}
    for n in range(len(f)):
        groups.setdefault(find(n), []).append(n)
    comps = []
    for members in groups.values():
        sub = f[members]
        edges = {(min(a, b), max(a, b)) for t in sub for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}
        closed = all(len(directed.get((a, b), [])) == 1 and len(directed.get((b, a), [])) == 1 for a, b in edges)
        comps.append(SimpleNamespace(faces=np.array(members), closed=closed, euler=len(np.unique(sub)) - len(edges) + len(sub)))
    return SimpleNamespace(manifold=manifold, components=comps)


def face_normals(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


# ---- fields for the extraction tests ----
def field(name, dims):
    """-> a namespace: origin (3,) float32, voxel_size float32, wsum, dsum (NZ,NY,NX) float32, csum (3,NZ,NY,NX) float32, value(x) and
    gradient(x) of the analytic field at points (n,3), spheres: how many closed surfaces the mesh has.  The planes hold
    dsum = fp32(w value), wsum = w with w in [1, 3): the quotient is not the value's own bits.
    names: sphere, plane (tilted, open at the grid's boundary), two_spheres, slab (the sphere with a layer of wsum = 0 through it),
    outside (positive everywhere), invalid (wsum = 0 everywhere)"""
    vs = np.float32(0.1)
    origin = np.array([-0.05 * (n - 1) + 0.013 for n in dims], np.float32) + np.float32(0.5)
    x = node_positions(dims, origin, vs)
    ext = 0.1 * (np.array(dims) - 1)
    centre = origin.astype(np.float64) + 0.5 * ext + np.array([0.021, -0.017, 0.011])
    if name in ("sphere", "slab", "invalid"):
        r = 0.36 * ext.min() + 0.0123
        value = lambda q: np.linalg.norm(q - centre, axis=1) - r
        gradient = lambda q: (q - centre) / np.linalg.norm(q - centre, axis=1, keepdims=True)
        spheres = 1
    elif name == "two_spheres":
        a = int(np.argmax(ext))
        c1, c2 = centre.copy(), centre.copy()
        c1[a] -= 0.25 * ext[a]
        c2[a] += 0.25 * ext[a]
        r = min(0.36 * np.delete(ext, a).min(), 0.2 * ext[a]) + 0.0041
        value = lambda q: np.minimum(np.linalg.norm(q - c1, axis=1), np.linalg.norm(q - c2, axis=1)) - r

        def gradient(q):
            n1, n2 = np.linalg.norm(q - c1, axis=1, keepdims=True), np.linalg.norm(q - c2, axis=1, keepdims=True)
            return np.where(n1 < n2, (q - c1) / n1, (q - c2) / n2)
        spheres = 2
    elif name == "plane":
        n = np.array([0.48, 0.31, 0.82])
        n /= np.linalg.norm(n)
        value = lambda q: (q - centre) @ n
        gradient = lambda q: np.broadcast_to(n, q.shape)
        spheres = 0
    elif name == "outside":
        value = lambda q: 0.3 + 0.0 * q[:, 0]
        gradient = lambda q: np.zeros_like(q)
        spheres = 0
    else:
        raise ValueError(name)
    rng = np.random.default_rng(dims[0] * 10000 + dims[1] * 100 + dims[2])
    shape = dims[::-1]
    w = (1.0 + 2.0 * rng.random(shape)).astype(np.float32)
    dsum = (w.astype(np.float64) * value(x).reshape(shape)).astype(np.float32)
    rgb = np.stack([0.5 + 0.5 * np.sin(3.0 * x[:, 0] + 1.0), 0.5 + 0.5 * np.cos(2.0 * x[:, 1]), 0.2 + 0.6 * (x[:, 2] - x[:, 2].min()) / max(ext[2], 0.1)])
    csum = (w.astype(np.float64)[None] * rgb.reshape((3,) + shape)).astype(np.float32)
    if name == "slab":
        w[:, :, dims[0] // 2] = 0.0
    if name == "invalid":
        w[:] = 0.0
    return SimpleNamespace(dims=dims, origin=origin, voxel_size=vs, wsum=w, dsum=dsum, csum=csum, value=value, gradient=gradient, spheres=spheres)


NOISE_SEED = 5
THRESHOLD = 2.0   # the min_weight at which the planted nodes of `noise` sit: wsum = 2.0 is valid, the float32 below it is not
# the scan's seams (tests/test_tsdf_gpu.py): 4 224 count workgroups of 256 nodes, a z layer is 64 of them and a workgroup two y rows
SEAM_DIMS, SEAM_ROWS, SEAM_LAYERS = (128, 128, 66), tuple(range(0, 8)) + tuple(range(120, 128)), (0, 1, 3, 4, 5, 7, 8, 15, 16, 62, 63, 64, 65)
WAVE_SEAM_DIMS = (65, 64, 17)   # 277 workgroups, every one with counts: the scan's first wave seam under dense data


def noise(dims, seed=NOISE_SEED, where=None):
    """A field without any smoothness, for the tables and the validity logic -> the namespace of `field` (without value and gradient),
    and planted_valid, planted_invalid: (4, 2) arrays of (node, its +x neighbour).
    wsum = fp32(1 + 2 u), u uniform in [0, 1); value i.i.d. uniform in (-1, 1); dsum = fp32(w value); then 5 % of the nodes get
    dsum = +0.0 and another 5 % dsum = -0.0: "outside", with their vertices on the node itself (t = 0 or 1).  At min_weight = THRESHOLD
    about half the nodes are invalid, scattered.  Planted: four nodes with wsum = THRESHOLD exactly and four with the float32 just below
    it, each with a +x neighbour of wsum >= THRESHOLD and dsum != 0 (none of them planted) and a value of the other sign: the edge between
    them is a vertex exactly where the comparison is >=.
    where (NZ, NY, NX) bool or None: outside it the field is the constant +0.3 of field("outside") -- valid, and no crossing between two
    such nodes."""
    vs = np.float32(0.1)
    origin = np.array([-0.05 * (n - 1) + 0.013 for n in dims], np.float32) + np.float32(0.5)
    x = node_positions(dims, origin, vs)
    ext = 0.1 * (np.array(dims) - 1)
    shape = dims[::-1]
    rng = np.random.default_rng(seed)
    w = (1.0 + 2.0 * rng.random(shape)).astype(np.float32)
    value = rng.uniform(-1.0, 1.0, shape)
    if where is not None:
        value = np.where(where, value, 0.3)
    dsum = (w.astype(np.float64) * value).astype(np.float32)
    r = rng.random(shape)
    if where is not None:
        r = np.where(where, r, 1.0)
    dsum[r < 0.05] = 0.0
    dsum[(r >= 0.05) & (r < 0.10)] = -0.0
    # the planted nodes, drawn from a shuffle of the nodes that have a +x neighbour
    NX = dims[0]
    wf, df = w.reshape(-1), dsum.reshape(-1)
    used, planted = set(), []
    noisy = np.ones(wf.size, bool) if where is None else where.reshape(-1)
    for n in (int(n) for n in rng.permutation(wf.size)):
        if len(planted) == 8:
            break
        if n % NX == NX - 1 or not noisy[n] or n in used or n + 1 in used or not wf[n + 1] >= np.float32(THRESHOLD) or df[n + 1] == 0:
            continue
        used.update((n, n + 1))   # neither a planted node nor its witness is touched again
        wf[n] = np.float32(THRESHOLD) if len(planted) < 4 else np.nextafter(np.float32(THRESHOLD), np.float32(0.0))
        df[n] = np.float32(float(wf[n]) * (-0.4 if df[n + 1] > 0 else 0.4))
        planted.append((n, n + 1))
    assert len(planted) == 8
    rgb = np.stack([0.5 + 0.5 * np.sin(3.0 * x[:, 0] + 1.0), 0.5 + 0.5 * np.cos(2.0 * x[:, 1]), 0.2 + 0.6 * (x[:, 2] - x[:, 2].min()) / max(ext[2], 0.1)])
    csum = (w.astype(np.float64)[None] * rgb.reshape((3,) + shape)).astype(np.float32)
    return SimpleNamespace(dims=dims, origin=origin, voxel_size=vs, wsum=w, dsum=dsum, csum=csum, spheres=0,
                           planted_valid=np.array(planted[:4], np.int64), planted_invalid=np.array(planted[4:], np.int64))


def seam_field():
    """noise in the rows SEAM_ROWS of the layers SEAM_LAYERS of SEAM_DIMS, the constant outside value elsewhere: counts on both sides of
    workgroups 255 | 256 and 511 | 512 (threads 63 | 64 and 127 | 128 of the plan's scan), 1 023 | 1 024, 4 095 | 4 096 (its second trip,
    with the carry) and in the last workgroup that holds a whole cell; nothing at all in the layers between."""
    where = np.zeros(SEAM_DIMS[::-1], bool)
    for k in SEAM_LAYERS:
        where[k, list(SEAM_ROWS), :] = True
    return noise(SEAM_DIMS, where=where)


def workgroup_counts(m, dims, threads=256):
    """-> (vertices, triangles) of the mesh `m` per count workgroup: node or cell index // threads"""
    groups = (dims[0] * dims[1] * dims[2] + threads - 1) // threads
    return np.bincount(m.node // threads, minlength=groups), np.bincount(m.cell // threads, minlength=groups)


def seam_layout(m, dims=SEAM_DIMS):
    """The conditions on the seam volume's reference mesh that make it a test of the scan, asserted; -> (vertices, triangles) per
    workgroup.  A scan thread takes 4 totals, a wave 256, a trip 4 096."""
    v, f = workgroup_counts(m, dims)
    groups = len(v)
    assert groups > 4096
    last = (dims[0] * (dims[1] - 2 + dims[1] * (dims[2] - 2))) // 256   # the workgroup of the last cell's node
    for g in (255, 256, 511, 512, 4095, 4096, last):
        assert v[g] > 0 and f[g] > 0, (g, v[g], f[g])
    assert last > 4096 and bool((f[4097:] > 0).any())                   # the carry feeds F as well as V
    quiet = (v == 0) & (f == 0)
    runs = np.diff(np.flatnonzero(np.diff(np.concatenate(([0], quiet.view(np.int8), [0])))))[::2]
    assert runs.size and int(runs.max()) >= 64                          # a stretch of the prefix that must stay flat
    assert len(m.vertices) < 400000 and len(m.faces) < 400000
    return v, f


# ---- the end-to-end scene: six cameras around an analytic sphere ----
SPHERE = SimpleNamespace(radius=0.5, dims=(24, 24, 24), half=0.8, W=64, H=64, distance=3.0, focal=100.0, trunc_voxels=3.0)


def sphere_scene():
    """-> (origin, voxel_size, rec (6,20), depth (6,H,W)) float32: cameras on the six axes at SPHERE.distance looking at the centre of a
    sphere of SPHERE.radius at the origin; depth = the z-depth of the exact ray intersection at pixel centres, 0 where the ray misses."""
    s = SPHERE
    vs = np.float32(2.0 * s.half / (s.dims[0] - 1))
    origin = np.full(3, -s.half, np.float32)
    recs, depths = [], []
    for axis in range(3):
        for sign in (1.0, -1.0):
            pos = np.zeros(3)
            pos[axis] = sign * s.distance
            rec = look_at(pos, (0, 0, 0), s.W, s.H, s.focal, up=(0.0, 0.0, 1.0) if axis == 1 else (0.0, 1.0, 0.0))
            r = rec.astype(np.float64)
            R, fx, fy, cx, cy = r[:9].reshape(3, 3), r[12], r[13], r[14], r[15]
            uu, vv = np.meshgrid(np.arange(s.W) + 0.5, np.arange(s.H) + 0.5)
            ray = np.stack([(uu - cx) / fx, (vv - cy) / fy, np.ones_like(uu)], axis=-1)   # camera space, z = 1
            o = -(R.T @ r[9:12])                                                           # the camera's centre in world space
            dirs = ray @ R                                                                 # world space
            a, b, c = (dirs * dirs).sum(-1), 2.0 * (dirs @ o), float(o @ o) - s.radius ** 2
            disc = b * b - 4 * a * c
            z = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0.0)    # the ray's parameter is the z-depth
            recs.append(rec)
            depths.append(z.astype(np.float32))
    return origin, vs, np.stack(recs), np.stack(depths)
