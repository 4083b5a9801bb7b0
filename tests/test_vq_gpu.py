"""GPU: the vector quantisation (include/gsr_vq.h, fused_vq) against the float64 reference tests/torch_vq.py, whose fixtures
tests/test_vq_cpu.py checks.  Integer grids with many exact ties pin the MFMA's lane map, the zero padding, the combine across lane
halves, LDS tiles and workgroups and the tie rule: idx and dist2 are exact there.  On general data every row satisfies
d2_true(idx) <= min_j d2_true(j) + E_chosen + E_best, with E the error of the 2 D-long float32 chain, and on separated clusters idx is
the float64 argmin.  The update is held to the bound of a double sum and one rounding, k-means to the reference's indices after every
iteration, everything to equal bits on a second call.  Raw calls write into buffers with canary elements behind them.

Recorded on the MI355X.  General cases (N, D, K, seed, offset) = (1200, 3, 200), (1000, 7, 129), (900, 45, 300), (800, 45, 130, offset 50),
(600, 64, 64): no row off the float64 argmin, so the largest ratio of d2_true(idx) - min_j d2_true(j) to E_chosen + E_best is 0 in all
five (the bound is the worst case of 2 D roundings that all push one way; a near-tie inside it did not occur at these sizes); dist2
within 0.973, 0.955, 0.902, 0.963, 0.894 of one rounding.  Update: 0.58 to 0.99 of the derived bound on lists below 512 members (one wave, sequential).  Offset 50 through k-means:
centred 0 of 3000 rows off the reference, not centred 1 (inside the raw rows' bound).  K = 64 end to end: 19.8 dB against the
unquantised render of the 2 000-Gaussian scene (recorded, not asserted)."""
import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import torch_vq as tv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 64          # canary elements behind every output of a raw call
CANARY = -777


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def raw_assign(x, c):
    """gsr_vq_assign on outputs with canaries behind them -> (idx, dist2) numpy"""
    import fused_vq as fv
    N, D = x.shape
    K = c.shape[0]
    xd, cd = dev(x), dev(c)
    idx = torch.full((N + GUARD,), CANARY, dtype=torch.int32, device=DEV)
    d2 = torch.full((N + GUARD,), float(CANARY), dtype=torch.float32, device=DEV)
    scratch = torch.empty((fv._lib().gsr_vq_assign_scratch_bytes(N, D, K),), dtype=torch.uint8, device=DEV)
    fv._run("gsr_vq_assign", N, D, xd.data_ptr(), K, cd.data_ptr(), idx.data_ptr(), d2.data_ptr(), scratch.data_ptr(),
            torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert bool((idx[N:] == CANARY).all()) and bool((d2[N:] == CANARY).all()), "a write behind the outputs"
    return idx[:N].cpu().numpy(), d2[:N].cpu().numpy()


# ---- integer grids: exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", tv.INTEGER_D)
def test_integer_grid_is_exact(D):
    import fused_vq as fv
    for K in tv.INTEGER_K:
        for N in tv.INTEGER_N:
            x, c = tv.integer_case(N, D, K, 1000 * D + K + N)
            want_idx, want_d2 = tv.integer_answer(x, c)
            idx, d2 = raw_assign(x, c)
            bad = np.flatnonzero(idx != want_idx)
            assert bad.size == 0, f"D {D} K {K} N {N}: {bad.size} rows differ, first {bad[:5]}: got {idx[bad[:5]]} want {want_idx[bad[:5]]}"
            assert np.array_equal(d2, want_d2), f"D {D} K {K} N {N}: dist2"
    i2, d22 = fv.assign(dev(x), dev(c))   # the public call gives the raw call's bits
    assert np.array_equal(i2.cpu().numpy(), idx) and np.array_equal(d22.cpu().numpy(), d2)


def test_lane_map_with_an_asymmetric_codebook():
    """code j = j e_(j mod D) scaled so that row i = code i exactly: a row / column swap or a wrong k half cannot pass"""
    D, K = 5, 160
    c = np.zeros((K, D), np.float32)
    for j in range(K):
        c[j, j % D] = 1 + j // D
        c[j, (j + 1) % D] = -(j % 7)
    x = c[::-1].copy()
    idx, d2 = raw_assign(x, c)
    want, wd2 = tv.integer_answer(x, c)
    assert np.array_equal(idx, want) and np.array_equal(d2, wd2) and np.all(d2 == 0)


# ---- general data: every row inside the derived bound ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def general():
    out = {}
    for case in tv.GENERAL:
        x, c = tv.general_case(*case)
        out[case] = (x, c) + tv.assign_ref(x, c) + (tv.score_error(x, c),)
    return out


@pytest.mark.parametrize("case", tv.GENERAL)
def test_general_data_every_row_within_the_score_error(general, case):
    x, c, ref_idx, ref_d2, m, E = general[case]
    idx, d2 = raw_assign(x, c)
    r = np.arange(len(x))
    assert idx.min() >= 0 and idx.max() < len(c)
    excess = m[r, idx] - ref_d2
    bound = E[r, idx] + E[r, ref_idx]
    print(f"case {case}: rows off the float64 argmin {int((idx != ref_idx).sum())}, largest excess / bound {float((excess / bound).max()):.3e}")
    assert np.all(excess <= bound)
    err = np.abs(d2.astype(np.float64) - m[r, idx])
    print(f"case {case}: largest dist2 error / one rounding {float((err / tv.dist2_rounding(m[r, idx], x.shape[1])).max()):.3f}")
    assert np.all(err <= tv.dist2_rounding(m[r, idx], x.shape[1]))


@pytest.mark.parametrize("case", tv.SEPARATED)
def test_separated_clusters_equal_the_float64_argmin(case):
    x, c, label = tv.separated_case(*case)
    idx, d2 = raw_assign(x, c)
    assert np.array_equal(idx, label)
    want = tv.dist2_true(x, c)[np.arange(len(x)), label]
    assert np.all(np.abs(d2 - want) <= tv.dist2_rounding(want, x.shape[1]))


# ---- special values ------------------------------------------------------------------------------------------------------------------
def test_duplicated_codes_nan_rows_and_overflow():
    x, c = tv.general_case(300, 7, 140, 41)
    c[130] = c[3]; c[77] = c[3]; c[139] = c[138]                       # the lower index of a duplicate wins
    x[5] = c[3]; x[6] = c[138]; x[200] = c[3]
    x[17, 2] = np.nan; x[299, :] = np.nan
    idx, d2 = raw_assign(x, c)
    ref_idx, ref_d2, m = tv.assign_ref(x, c)
    assert idx[5] == 3 and idx[200] == 3 and idx[6] == 138 and d2[5] == 0 and d2[6] == 0
    assert not np.isin(idx, [77, 130, 139]).any()
    assert idx[17] == -1 and idx[299] == -1 and np.isnan(d2[17]) and np.isnan(d2[299])
    ok = ~np.isnan(x).any(axis=1)
    E = tv.score_error(x[ok], c)
    r = np.arange(int(ok.sum()))
    assert np.all(m[ok][r, idx[ok]] - ref_d2[ok] <= E[r, idx[ok]] + E[r, ref_idx[ok]])
    # every score overflows: |c|^2 = +inf in float32 and the chain stays there
    big = np.full((130, 7), 1e20, np.float32)
    idx, d2 = raw_assign(x[:70], big)
    assert np.all(idx == -1) and np.all(np.isnan(d2))
    # one finite code among them is found wherever it stands
    for j in (0, 64, 129):
        big2 = big.copy(); big2[j] = 0.5
        idx, _ = raw_assign(x[20:90], big2)
        assert np.all(idx == j)


def test_largest_codebook():
    x, c = tv.general_case(130, 3, 65536, 43)
    idx, d2 = raw_assign(x, c)
    ref_idx, ref_d2, m = tv.assign_ref(x, c)
    E = tv.score_error(x, c)
    r = np.arange(len(x))
    assert np.all(m[r, idx] - ref_d2 <= E[r, idx] + E[r, ref_idx])
    c[65535] = x[7]; c[65000] = x[8]
    idx, d2 = raw_assign(x, c)
    assert idx[7] == 65535 and idx[8] == 65000 and d2[7] == 0


def test_strided_inputs_give_the_contiguous_bits():
    import fused_vq as fv
    x, c = tv.general_case(700, 45, 200, 44)
    xw = torch.zeros((700, 2, 64), device=DEV); xw[:, 1, 3:48] = dev(x)
    cw = torch.zeros((45, 400), device=DEV); cw[:, ::2] = dev(c).t()
    xs, cs = xw[:, 1, 3:48], cw[:, ::2].t()
    assert not xs.is_contiguous() and not cs.is_contiguous()
    a, b = fv.assign(dev(x), dev(c)), fv.assign(xs, cs)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    w = torch.rand(700, device=DEV)
    u1, u2 = fv.update(dev(x), a[0], dev(c), w), fv.update(xs, a[0], cs, w.repeat_interleave(2)[::2])
    assert all(torch.equal(p, q) for p, q in zip(u1, u2))


# ---- update ----------------------------------------------------------------------------------------------------------------------
def raw_update(x, idx, c, w):
    """gsr_vq_update through the graph build, outputs with canaries behind them -> (codebook, count, wsum) numpy"""
    import fused_knn as fk
    import fused_vq as fv
    N, D = x.shape
    K = c.shape[0]
    graph = fk.NeighborGraph(dev(idx)[:, None], K)
    xd = dev(x)
    wd = None if w is None else dev(w)
    cb = torch.full((K * D + GUARD,), float(CANARY), dtype=torch.float32, device=DEV)
    cb[:K * D] = dev(c).reshape(-1)
    count = torch.full((K + GUARD,), CANARY, dtype=torch.int32, device=DEV)
    wsum = torch.full((K + GUARD,), float(CANARY), dtype=torch.float32, device=DEV)
    fv._run("gsr_vq_update", N, D, xd.data_ptr(), None if wd is None else wd.data_ptr(), K, graph.offsets.data_ptr(), graph._edges.data_ptr(),
            cb.data_ptr(), count.data_ptr(), wsum.data_ptr(), torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert bool((cb[K * D:] == CANARY).all()) and bool((count[K:] == CANARY).all()) and bool((wsum[K:] == CANARY).all()), "a write behind the outputs"
    return cb[:K * D].reshape(K, D).cpu().numpy(), count[:K].cpu().numpy(), wsum[:K].cpu().numpy()


def _check_update(x, idx, c, w):
    import fused_vq as fv
    new, count, W, bound = tv.update_ref(x, idx, c, w)
    got, gcount, gw = raw_update(x, idx, c, w)
    assert np.array_equal(gcount, count)
    assert np.all(np.abs(gw.astype(np.float64) - W) <= tv.U * W + (count + 2.0) * 2.0 ** -53 * W)
    err = np.abs(got.astype(np.float64) - new)
    moved = bound[:, 0] > 0
    print(f"update N {len(x)} D {x.shape[1]} K {len(c)}: codes moved {int(moved.sum())}, largest error / bound "
          f"{float((err[moved] / bound[moved]).max()) if moved.any() else 0.0:.3f}")
    assert np.all(err <= bound)
    assert np.array_equal(got[~moved].view(np.int32), c[~moved].view(np.int32))   # kept bit for bit
    pub = fv.update(dev(x), dev(idx), dev(c), None if w is None else dev(w))
    assert np.array_equal(pub[0].cpu().numpy().view(np.int32), got.view(np.int32))
    assert np.array_equal(pub[1].cpu().numpy(), gcount) and np.array_equal(pub[2].cpu().numpy(), gw)
    return got


@pytest.mark.parametrize("N,D,K,seed", [(3000, 45, 70, 51), (2000, 7, 300, 52), (1000, 64, 5, 53), (777, 1, 9, 54), (900, 3, 130, 55)])
@pytest.mark.parametrize("weighted", [False, True])
def test_update_against_the_reference(N, D, K, seed, weighted):
    rng = np.random.default_rng(seed)
    x, c = tv.general_case(N, D, K, seed, offset=3.0)
    c[0, 0] = -0.0
    idx = rng.integers(-1, K, N).astype(np.int32)            # -1: rows that belong to no code
    idx[idx == 0] = 1 if K > 1 else 0                         # code 0 stays empty where there is another
    if K > 4:
        idx[idx == 4] = 3
        idx[10] = 4                                           # one member
    w = rng.uniform(0.0, 2.0, N).astype(np.float32) if weighted else None
    if weighted and K > 2:
        w[idx == 2] = 0.0                                     # members, but weights that add up to 0
    got = _check_update(x, idx, c, w)
    if K > 4:
        want = x[10] if w is None or w[10] > 0 else c[4]
        assert np.array_equal(got[4], want.astype(np.float32))   # the mean of one row is the row


def test_update_one_code_owns_every_row():
    x, c = tv.general_case(40000, 7, 3, 56, offset=50.0)
    idx = np.full(40000, 1, np.int32)
    _check_update(x, idx, c, None)
    _check_update(x, idx, c, np.random.default_rng(3).uniform(0, 1, 40000).astype(np.float32))


def test_update_list_lengths_around_the_split():
    """lists of 512 members and more are added in up to sixteen parts (include/gsr_vq.h): lengths either side of every change of the
    part count that the sizes here reach, and lengths that leave the last part short"""
    lengths = [1, 255, 256, 511, 512, 513, 767, 768, 1023, 1024, 1025, 2047, 2049, 3839, 3840, 4095, 4096, 4097, 5000]
    rng = np.random.default_rng(57)
    idx = np.concatenate([np.full(n, j, np.int32) for j, n in enumerate(lengths)] + [np.full(300, -1, np.int32)])
    rng.shuffle(idx)
    x, c = tv.general_case(len(idx), 5, len(lengths) + 1, 57, offset=10.0)
    _check_update(x, idx, c, None)
    _check_update(x, idx, c, rng.uniform(0, 3, len(idx)).astype(np.float32))


# ---- k-means ---------------------------------------------------------------------------------------------------------------------
def test_kmeans_on_separated_clusters_follows_the_reference():
    import fused_vq as fv
    N, D, K, seed = tv.KMEANS_SEPARATED
    x, c, _ = tv.separated_case(N, D, K, seed)
    w = np.random.default_rng(5).uniform(0.5, 2.0, N).astype(np.float32)
    for weight in (None, w):
        steps = tv.kmeans_ref(x, c, 3, weight)
        for t in range(1, 4):                                 # the state after every iteration
            cb, idx, inertia = fv.kmeans(dev(x), K, iters=t, init=dev(c), weight=None if weight is None else dev(weight))
            ref_idx, ref_cb, ref_in, _ = steps[t - 1]
            assert np.array_equal(idx.cpu().numpy(), ref_idx)
            # the update's bound on the centred rows, one rounding for adding the mean back, and the drift of the codebook the
            # iterations before assigned against does not enter: the indices are equal, so the members are
            bound = tv.update_ref(x, ref_idx, c, weight)[3] + 2 * tv.U * (np.abs(ref_cb) + np.abs(x).max(0)[None, :])
            assert np.all(np.abs(cb.cpu().numpy().astype(np.float64) - ref_cb) <= bound)
            got_in = inertia.cpu().numpy()
            assert got_in.shape == (t,) and got_in.dtype == np.float64
            # a coordinate of a centred row or code is off by at most delta (the centring's rounding, the codebook bound above), so
            # a squared distance by at most 2 |diff|_1 delta + D delta^2 <= 2 sqrt(D d2) delta + D delta^2; then one rounding of dist2
            d2 = tv.dist2_true(x, steps[t - 1][3])[np.arange(N), ref_idx]
            delta = 8 * tv.U * max(np.abs(x).max(), np.abs(c).max())
            ww = np.ones(N) if weight is None else weight.astype(np.float64)
            tol = float((ww * (2 * np.sqrt(D * d2) * delta + D * delta ** 2 + tv.dist2_rounding(d2, D))).sum())
            print(f"k-means iteration {t}: inertia {got_in[-1]:.9e} reference {ref_in:.9e} tolerance {tol:.3e}")
            assert abs(got_in[-1] - ref_in) <= tol


def test_kmeans_inertia_does_not_increase_and_centering_matters():
    import fused_vq as fv
    x, _ = tv.general_case(4000, 7, 1, 61)
    cb, idx, inertia = fv.kmeans(dev(x), 50, iters=8, seed=3)
    v = inertia.cpu().numpy()
    print("inertia:", v)
    # Lloyd's steps cannot raise the true inertia; the recorded one carries each dist2's rounding (2^-24 relative) and the
    # score-error slack of rows assigned off the true argmin, which the 1e-5 here covers with room
    assert np.all(v[1:] <= v[:-1] * (1 + 1e-5)) and v[-1] < 0.9 * v[0]
    assert cb.shape == (50, 7) and idx.shape == (4000,) and int(idx.min()) >= 0 and int(idx.max()) < 50
    # offset 50, spread 1: centred, the indices are the float64 reference's on the rows float64 itself can tell apart
    xo, co = tv.general_case(3000, 7, 40, 62, offset=50.0)
    ref_idx, _, m = tv.assign_ref(xo, co)
    mean = xo.astype(np.float64).mean(0).astype(np.float32)
    gap, need = tv.gaps(xo - mean, co - mean)
    _, idx_c, _ = fv.kmeans(dev(xo), 40, iters=1, init=dev(co), center=True)
    _, idx_u, _ = fv.kmeans(dev(xo), 40, iters=1, init=dev(co), center=False)
    sure = gap > 4 * need
    print(f"offset 50: rows float32 can tell apart when centred {int(sure.sum())} of 3000; off the reference centred "
          f"{int((idx_c.cpu().numpy() != ref_idx).sum())}, not centred {int((idx_u.cpu().numpy() != ref_idx).sum())}")
    assert sure.all()                                         # a property of the fixture: centred, float32 can tell every row's best
    assert np.array_equal(idx_c.cpu().numpy(), ref_idx)
    # not centred, the rule is still the score bound on the raw rows
    E = tv.score_error(xo, co)
    r = np.arange(3000)
    iu = idx_u.cpu().numpy()
    assert np.all(m[r, iu] - m[r, ref_idx] <= E[r, iu] + E[r, ref_idx])


# ---- reproducibility ----------------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bits():
    import fused_vq as fv
    x, c = tv.general_case(5000, 45, 300, 71)
    xd, cd = dev(x), dev(c)
    w = torch.rand(5000, device=DEV)
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)
    for call in (lambda: fv.assign(xd, cd), lambda: fv.update(xd, fv.assign(xd, cd)[0], cd, w), lambda: fv.kmeans(xd, 64, iters=3, weight=w, seed=1)):
        a, b = call(), call()
        assert all(torch.equal(bits(p), bits(q)) for p, q in zip(a, b))


def test_lookup_is_the_gather_with_a_fixed_order_backward():
    import fused_vq as fv
    x, c = tv.general_case(2000, 7, 33, 72)
    cd = dev(c).requires_grad_(True)
    idx = fv.assign(dev(x), cd)[0]
    rows = fv.lookup(cd, idx)
    assert torch.equal(rows.detach(), cd.detach()[idx.long()])
    up = dev(x)
    (rows * up).sum().backward()
    want = np.zeros((33, 7), np.float32)
    for i, j in enumerate(idx.cpu().numpy()):                 # the sequential float32 sum in ascending row order
        want[j] += x[i]
    assert np.array_equal(cd.grad.cpu().numpy(), want)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _render(pc, scene, cam):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    to = lambda t: t.to(DEV)
    settings = GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=to(scene.bg),
        scale_modifier=1.0, viewmatrix=to(cam.world_view_transform), projmatrix=to(cam.full_proj_transform), sh_degree=3,
        campos=to(cam.camera_center), prefiltered=False, debug=False)
    with torch.no_grad():
        color, _ = GaussianRasterizer(settings)(means3D=pc.get_xyz, means2D=torch.zeros_like(pc.get_xyz), shs=pc.get_features,
                                                opacities=pc.get_opacity, scales=pc.get_scaling, rotations=pc.get_rotation)
    return color


def test_quantised_model_renders_as_its_codebook_rows(tmp_path):
    import fused_vq as fv
    import gsr_model
    import gsr_scene
    scene = gsr_scene.make_scene(2000, -3.0, sh_degree=3, seed=3)
    cam = gsr_scene.make_camera(200, 120)
    pc = gsr_model.GaussianParams.from_activated(scene.means3D, scene.shs, scene.scales, scene.rotations, scene.opacities, device=DEV,
                                                 requires_grad=False)
    names = ("features_rest", "scaling", "rotation")
    importance = torch.rand(2000, device=DEV)
    vq = fv.quantize_gaussians(pc, {n: 64 for n in names}, importance=importance, iters=5, seed=2)
    assert set(vq.coded) == set(names) and all(vq.coded[n][0].shape[0] == 64 for n in names)
    rot = vq.coded["rotation"][0]
    assert torch.allclose(rot.norm(dim=1), torch.ones(64, device=DEV), atol=1e-6)
    path = str(tmp_path / "scene_vq.npz")
    vq.save(path)
    back = fv.VQGaussians.load(path, device=DEV)
    got = _render(back.dequantize(), scene, cam)
    # the same model assembled in plain torch
    leaves = {n: p.detach().clone() for n, p in zip(fv.LEAVES, pc.parameters())}
    for n in names:
        cb, idx = vq.coded[n]
        leaves[n] = cb[idx.long()].reshape(leaves[n].shape)
    want = _render(gsr_model.GaussianParams(*[leaves[n] for n in fv.LEAVES]), scene, cam)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    full = _render(pc, scene, cam)
    mse = float(((got - full) ** 2).mean())
    print(f"PSNR of the K = 64 model against the unquantised render: {10 * np.log10(1.0 / max(mse, 1e-30)):.2f} dB")
    again = fv.quantize_gaussians(pc, {n: 64 for n in names}, importance=importance, iters=5, seed=2)
    for n in names:
        assert torch.equal(again.coded[n][0].view(torch.int32), vq.coded[n][0].view(torch.int32)) and torch.equal(again.coded[n][1], vq.coded[n][1])
