"""CPU: the fixtures of the binning seam tests (tests/binning_cases.py) have the counts their names say, the numpy reference
agrees with the C oracle, and the comparison the GPU tests use detects every defect it is there for.

(a) keeps a case from silently missing its seam: each fixture's P, visible and culled counts, tiles touched per kind, column pairs,
    instances, pairs per tile column and depth-bucket sizes are asserted on the ORACLE's state -- a fixture off its seam is a failure.
(b) reference_binning on the oracle's rectangles and depths gives the oracle's point_list, keys and ranges.
(c) check_lists raises on swapped neighbours, a dropped or duplicated instance, a range off by one, an empty tile given (p, p) and a
    broken tie -- the stand-in for mutating the kernels, which on a GPU would turn into wild addresses."""
import numpy as np
import pytest

import binning_cases as bc

CPU_NAMES = [n for n in bc.A_NAMES + bc.B_NAMES + bc.C_NAMES + bc.D_SMALL_NAMES + [bc.D4_NAME] + bc.F_NAMES]


def test_the_cpu_file_covers_every_fixture_of_at_most_70000_gaussians():
    for n in CPU_NAMES:
        assert bc.case(n).P <= 70_000, n
    for n in bc.E_NAMES:
        assert int(n[2:]) > 70_000


def _columns(rect, gx):
    x0, w = rect[:, 0], rect[:, 2]
    g = np.repeat(np.arange(rect.shape[0]), w)
    c = x0[g] + np.arange(int(w.sum())) - np.repeat(np.cumsum(w) - w, w)
    return np.bincount(c, minlength=gx)


@pytest.mark.parametrize("name", CPU_NAMES)
def test_fixture_has_the_counts_its_name_says(name):
    c = bc.case(name)
    o = bc.oracle_state(name)
    e = c.expect
    W, H = c.cam.image_width, c.cam.image_height
    gx, gy = (W + 15) // 16, (H + 15) // 16
    assert o["P"] == e["P"] == c.P
    if "tiles" in e:
        assert gx * gy == e["tiles"]
    if name in bc.F_NAMES:
        assert o["num_rendered"] > 0 and int((o["radii"] > 0).sum()) > 1000
        return
    vis = o["radii"] > 0
    assert int(vis.sum()) == e["visible"] and int((~vis).sum()) == e["culled"]
    assert np.array_equal(vis, c.bits != bc.CULLED)
    # the depth is z + 4, exact in fp32: the oracle's depth bits are the chosen ones
    assert np.array_equal(o["depths"].view(np.uint32)[vis], c.bits[vis])
    rect = bc.rect_of_oracle(o)
    tt = o["tiles_touched"].astype(np.int64)
    assert np.array_equal(rect[:, 2] * rect[:, 3], tt)
    assert o["num_rendered"] == e["R"] == int(tt.sum())
    if "kinds" in e:
        got = {int(k): int(n) for k, n in zip(*np.unique(tt[vis], return_counts=True))}
        assert got == {k: n for k, n in e["kinds"].items() if n}
        if set(e["kinds"]) <= {1, 2, 4}:   # centres, seams, corners: 1, 2, 2 columns
            assert int(rect[:, 2].sum()) == e["kinds"].get(1, 0) + 2 * e["kinds"].get(2, 0) + 2 * e["kinds"].get(4, 0)
    if "shapes" in e:
        assert np.array_equal(rect[:, 2:4], e["shapes"])
    if "pairs" in e:
        assert int(rect[:, 2].sum()) == e["pairs"]
    if "col_pairs" in e:
        assert np.array_equal(_columns(rect, gx), e["col_pairs"])
    db = bc.depth_buckets(np.where(vis, o["depths"].view(np.uint32), bc.CULLED))
    if "top_shift" in e:
        assert db["top_shift"] == e["top_shift"] and db["range"] == e["range"]
    if "slab" in e:
        b, n = e["slab"]
        assert db["min"] == bc.F32_2_5 and int(db["sizes"][b]) == n, f"bucket {b} holds {int(db['sizes'][b])}"
        assert (bc.F32_4 - db["min"]) >> db["top_shift"] == b and (bc.F32_4 - db["min"]) & 0xFFFF == 0   # the slab's bucket starts at 4.0
    if "digit" in e:
        d, n = e["digit"]
        k = c.bits.astype(np.int64) - db["min"]
        assert int((((k >> 16) == bc.B_SLAB) & (((k >> 8) & 255) == d)).sum()) == n
    if "identical" in e:
        v, n = e["identical"]
        assert int((c.bits == v).sum()) == n
    if "consecutive" in e:
        n, span = e["consecutive"]
        pos = np.nonzero(tt[bc.reference_depth_order(c.bits)] == span)[0]
        assert len(pos) == n and pos[-1] - pos[0] == n - 1
    if "tile_span" in e:
        ne = np.nonzero(o["ranges"][:, 1] > o["ranges"][:, 0])[0]
        assert (int(ne[0]), int(ne[-1])) == e["tile_span"]
    if "straddle_min" in e:
        assert int((rect[:, 3] == 2).sum()) >= e["straddle_min"]
        lens = o["ranges"][:, 1].astype(np.int64) - o["ranges"][:, 0]
        assert lens[65536] >= e["last_tiles_min"] and lens[65537] >= e["last_tiles_min"]


@pytest.mark.parametrize("name", ["D2_middle_third", "C5_trim_words", "B_identical2049", "D3_257_tiles"])
def test_reference_binning_equals_the_oracle(name):
    """Between them: empty leading and trailing tiles, multi-tile rectangles, equal depths, more than 256 tile columns."""
    c, o = bc.case(name), bc.oracle_state(name)
    gx, gy = (c.cam.image_width + 15) // 16, (c.cam.image_height + 15) // 16
    bits = np.where(o["radii"] > 0, o["depths"].view(np.uint32), bc.CULLED)
    want = bc.reference_binning(bc.rect_of_oracle(o), bits, gx, gy)
    bc.check_lists(o, want, name)
    assert np.array_equal(bc.reference_depth_order(bits), np.lexsort((np.arange(c.P), bits)))


def _good(name):
    c, o = bc.case(name), bc.oracle_state(name)
    gx, gy = (c.cam.image_width + 15) // 16, (c.cam.image_height + 15) // 16
    w = bc.reference_binning(bc.rect_of_oracle(o), c.bits, gx, gy)
    bc.check_lists(w, w)
    return w, {k: v.copy() for k, v in w.items()}


def _without(a, p):
    return np.concatenate([a[:p], a[p + 1:]])


def test_checker_detects_swapped_neighbours_at_a_block_seam():
    want, got = _good("D2_tile0")   # 2 000 instances in tile 0
    for k in ("point_list", "keys"):
        got[k][[1023, 1024]] = got[k][[1024, 1023]]
    with pytest.raises(AssertionError, match=r"position 1023 \(tile 0\)"):
        bc.check_lists(got, want)


def test_checker_detects_a_dropped_and_a_duplicated_instance():
    want, got = _good("D2_tile0")
    drop = dict(point_list=_without(got["point_list"], 1024), keys=_without(got["keys"], 1024), ranges=got["ranges"].copy())
    drop["ranges"][0, 1] -= 1
    with pytest.raises(AssertionError, match=r"position 1024 \(tile 0\)"):
        bc.check_lists(drop, want)
    dup = dict(point_list=np.insert(got["point_list"], 1024, got["point_list"][1023]), keys=np.insert(got["keys"], 1024, got["keys"][1023]),
               ranges=got["ranges"].copy())
    dup["ranges"][0, 1] += 1
    with pytest.raises(AssertionError, match=r"position 1024 \(tile 0\)"):
        bc.check_lists(dup, want)
    # ... and when the very last instance is the one missing
    last = dict(point_list=got["point_list"][:-1], keys=got["keys"][:-1], ranges=got["ranges"])
    with pytest.raises(AssertionError, match="1999 entries, expected 2000"):
        bc.check_lists(last, want)


def test_checker_detects_a_range_off_by_one_and_a_non_zero_empty_range():
    want, got = _good("D2_middle_third")
    got["ranges"][100, 1] += 1
    with pytest.raises(AssertionError, match="range of tile 100"):
        bc.check_lists(got, want)
    want, got = _good("D2_middle_third")
    assert tuple(want["ranges"][200]) == (0, 0) and tuple(want["ranges"][3]) == (0, 0)
    got["ranges"][200] = (2000, 2000)   # an empty trailing tile given (p, p), as a scan without the reference's zero fill would leave it
    with pytest.raises(AssertionError, match="range of tile 200"):
        bc.check_lists(got, want)
    want, got = _good("D2_middle_third")
    got["ranges"][3] = (0, 0)
    got["ranges"][4] = (7, 7)
    with pytest.raises(AssertionError, match="range of tile 4"):
        bc.check_lists(got, want)


def test_checker_detects_equal_depths_in_descending_index_order():
    want, got = _good("B_identical2049")
    eq = np.nonzero(want["keys"][1:] == want["keys"][:-1])[0]
    assert eq.size >= 2048
    p = int(eq[0])
    assert want["point_list"][p] < want["point_list"][p + 1]     # ties are in ascending index order
    got["point_list"][[p, p + 1]] = got["point_list"][[p + 1, p]]   # (the keys are equal: only the ids change)
    with pytest.raises(AssertionError, match=f"point_list .* position {p} "):
        bc.check_lists(got, want)
