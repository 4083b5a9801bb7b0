"""GPU: the backward blend's per-Gaussian sums held to a float64 bound ROW BY ROW, on scenes whose small rows are the workload.

The norm-wise bars of test_parity_gpu.check_grads (max|d| <= 1e-5 max|g| per tensor) speak for the few Gaussians with the largest
gradients; Adam and the densification consume each row by itself.  check_grads therefore starts with a per-row level
(test_parity_gpu.check_rows): every row and component of the HIP blend sums dL_dmeans2D, dL_dconic, dL_dopacity, dL_dcolors within

    |hip - S| <= E = 2^-24 (B + n A),

S the float64 sum with the fp32 path's decisions (oracle.blend_backward_budget, oracle/gsr_oracle.c), n the number of (pixel,
Gaussian) terms of the row, A = sum |term|, B = the sum of the per-term budgets below; rows with n = 0 hold +0 bits.

Derived, not measured.  u = 2^-24, first order in u (the relative budgets stay below 2^-10, the neglected products below a
thousandth of what is kept, and every count below is rounded up to the form with more roundings of backward.cu:507-599 and
csrc/render_backward.hip).  dx, dy are fp32 differences that the float64 reference takes over as they are.
  n A     a sum of n fp32 values in ANY order errs by at most (n - 1) u sum |value|: the reference's atomics, the kernels' lane sums,
          LDS tree, slot sum and wave reduction are such orders (adding an exact zero is exact).  For dL/dmean2D, A is the sum of the
          moduli of the term's two products, |a f dx| + |b f dy|, not of the term: the kernel adds the moments sum f dx, sum f dy and
          applies the conic to the sums, and there the two products cancel only after the accumulation.
  power   -0.5 (a dx dx + c dy dy) - b dx dy: each of the three products has two roundings, 2 u pm together with
          pm = (|a| dx^2 + 2 |b dx dy| + |c| dy^2) / 2, the mass of `power`; the two sums one rounding each of at most u pm: 4 u pm.
  G       G's relative error is power's absolute error.  The blend kernels call __expf (render_forward.hip; render_backward.hip
          spells it v_exp_f32(power * log2(e))): the product with the rounded constant adds 2 u |power| <= 2 u pm, the instruction
          is accurate to 1 ulp = 2 u (the oracle's expf: below 1 ulp).  dG = (6 pm + 2) u.
  alpha   min(0.99f, o G): one product, dal = dG + u.  1 - alpha: absolute alpha dal + u (1 - alpha), so relative
          doma = alpha / (1 - alpha) dal + u.
  T       the weight of the contributor index.  final_T is the forward's product of (1 - alpha_j) over every hit of the pixel, one
          rounding each: dTfinal = sum_j (doma_j + u).  The backward rebuilds T by one division per hit from the back,
          T / (1 - alpha) as reciprocal (1 ulp) times T: dT_i = dTfinal + sum_{j >= i} (doma_j + 3 u).  (No use is made of the
          forward and the backward meeting the same bits of alpha, which would cancel the doma_j of the hits behind.)
  accum_rec  absolute error e per channel: e' = (1 - alpha) e + alpha dal |c - accum_rec| + u (2 alpha |c| + max(1, 3 (1 - alpha))
          |accum_rec|): the larger of the reference's two products, difference and sum and of the kernel's difference and FMA.
  dL/dalpha  = T sum_ch (c - accum_rec) dL/dpix + (-T_final / (1 - alpha)) (bg . dL/dpix).  With S1 the modulus of the first part,
          M1 = T sum_ch |(c - accum_rec) dL/dpix| and M2 = T_final / (1 - alpha) sum_ch |bg dL/dpix|:
          EA = T sum_ch e_ch |dL/dpix_ch| + dT S1 + 7 u M1 + (dTfinal + doma + 8 u) M2  (difference, product, two sums, the product
          with T, the last sum, one spare; three for bg . dL/dpix, the product with T_final, reciprocal and product, the last sum).
  terms   colour alpha T dL/dpix: (dal + dT + 2 u) |term|.  opacity G dL/dalpha: G (EA + (dG + u) MA), MA = M1 + M2.
          conic -0.5 G dx dx o dL/dalpha (and dx dy, dy dy): g (EA + (dG + 4 u) MA) with g = 0.5 o G dx^2 (...): four products.
          mean2D o dL/dalpha (-G dx a - G dy b) 0.5 W: g (EA + (dG + 6 u) MA) with g = 0.5 W o G (|a dx| + |b dy|): five products
          and a sum along any path, in the reference's form and in the kernel's (three of them after the sum).
  restart the one operation the kernels do differently, found by this level: the first run of the 40 000-Gaussian heavy scene of
          tests/test_backward_flush_gpu.py left 2 027 / 5 279 / 1 744 rows and components of dL_dmeans2D / dL_dconic / dL_dopacity
          outside the bound above, by up to 49 E (Gaussian 95, one term: dL_dopacity -1.4307614e-06 against -1.4275834e-06), with
          dL_dcolors at 0.07 E: T was right and accum_rec was not.  A depth segment of a heavy tile (csrc/render_backward.hip) starts
          its walk from the forward's checkpoint, accum_rec = (C_final - C) / T with C the forward's fp32 colour sum before the
          segment's last position -- a difference of two sums instead of the reference's recurrence (tests/test_boundary_gpu.py names it).
          C_final continues C by one FMA per hit behind: each rounds by at most u |C| <= u C_abs, C_abs = sum |c| alpha T over the
          pixel, and its addend c (alpha T) carries alpha's and the forward T's relative error and one rounding.  With dD the sum of
          these over the hits behind, the restarted value errs by dD / T + |accum_rec| (dTfinal + 3 u) (difference, reciprocal,
          product, T's own error).  At the first hit in front of a position where a walk may start -- every 512th
          (GSR_CKPT_STRIDE) position of the list the binning kept, which check_rows takes from the kernels' own trim words --
          e = max(e, that), and the recurrence goes on from there.  It is a worst case that grows with the hits behind, the price
          of restarting: tests/test_grad_rows_cpu.py prints what it costs the heavy fixture's bound.
The oracle's own fp32 results (accum_mode 0, 1, 2) stay inside E on every case and fixture: tests/test_grad_rows_cpu.py, which also
holds the fixtures to "E <= 1e-3 |S| on 90 % of the rows" and shows that the norm-wise bars miss defects of small rows.

Fixtures (tests/grad_rows.py), each run twice for the same bits, under grad_rows.smooth_dpix:
  slot runs   421 Gaussians on 512 x 128: tiles_touched takes each of 1, 2, 5, 6, 7, 12, 13, 29, 30, 31, 32, 62, 64, 65, 128 with
              slot_base at each residue mod 4 (csrc/gaussian_backward.hip: a lane adds runs of up to GSR_SLOT_COOP = 30 slots in
              rounds of GSR_SLOT_ROUND = 6, the wave adds longer ones, validity bytes come as aligned dwords at any byte offset);
              with the trim, which leaves invalid slots inside the runs of the large splats, and with GSR_DEBUG_NO_TRIM.
  deep tile   200 Gaussians of opacity 0.3 ... 0.6 on one tile: every walk ends on n_contrib, the rows span eight decades.
  heavy       the blob of test_backward_flush_gpu._heavy_scene at 3 200 Gaussians on 144 x 144: the blob falls on the centre tile, a
              list of more than 4 x 512 instances; 81 tiles, because below 64 the dispatch cuts no walk and splits no tile
              (csrc/binning.hip).  Walked in depth segments and split in bands, and whole with GSR_DEBUG_NO_SPLIT.

Largest err / E per tensor (dL_dmeans2D, dL_dconic, dL_dopacity, dL_dcolors), printed by the tests:
  the oracle's fp32, all cases and fixtures of the CPU file      0.050  0.076  0.074  0.089
  the kernels on the MI355X: slot runs (both ways)               0.018  0.027  0.020  0.040
                             deep tile                            0.020  0.022  0.018  0.036
                             heavy, split (walks restarted)       0.117  0.141  0.141  0.067
                             heavy, whole                         0.021  0.035  0.034  0.067
                             every caller of check_grads          0.447  0.486  0.486  0.135
  (the largest on the scenes whose walks restart: the heavy scenes of test_backward_flush_gpu.py and test_fuzz_gpu.py; 0.13 at most
  on scenes without a restart)
"""
import numpy as np
import pytest
import torch

import grad_rows as gr
import util
from test_parity_gpu import check_forward, check_grads

pytestmark = pytest.mark.gpu
GRADS = ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), f"{what}: two runs differ"


def _check_twice(scene, cam, D, label, debug=False):
    """The full check_grads of one run (per row, blend, chain, end to end), then a second run with the same bits."""
    o = util.oracle_forward(scene, cam, D)
    dpix = gr.smooth_dpix(o, cam)
    h = util.hip_forward_backward(scene, cam, D, dpix, debug=debug)
    check_forward(h, o, cam)
    check_grads(h, o, dpix, GRADS, label=label)
    h2 = util.hip_forward_backward(scene, cam, D, dpix, debug=debug)
    _same_bits(h["color"], h2["color"], "color")
    for k in h["raw_grads"]:
        _same_bits(h["raw_grads"][k], h2["raw_grads"][k], k)
    for k in h["grads"]:
        _same_bits(h["grads"][k], h2["grads"][k], k)
    return o, h, dpix


@pytest.mark.parametrize("trim", ["trimmed", "whole_lists"])
def test_slot_runs(trim):
    _need_gpu()
    from diff_gaussian_rasterization import _C
    scene, cam, runs = gr.slot_runs_scene()
    o, h, _ = _check_twice(scene, cam, 0, f"slot runs/{trim}", debug=_C.DEBUG_NO_TRIM if trim == "whole_lists" else False)
    gr.assert_slot_runs(h["tiles_touched"], runs)
    tt = h["tiles_touched"].astype(np.int64)
    np.testing.assert_array_equal(h["slot_base"], (np.cumsum(tt) - tt).astype(np.uint32))
    listed = len(h["point_list"])
    if trim == "trimmed":
        assert listed < o["num_rendered"], "nothing was trimmed: no invalid slot inside a run by the trim"
        big = [i for (L, _), i in runs.items() if L >= 62]
        assert (h["rshape"][big, 1] != 0).any(), "no large splat carries a trim word"
    else:
        assert listed == o["num_rendered"]


def test_one_deep_tile():
    _need_gpu()
    scene, cam = gr.deep_tile_scene()
    o, h, dpix = _check_twice(scene, cam, 0, "deep tile")
    gr.assert_deep_tile(o, util.oracle.blend_backward_budget(o, dpix.numpy()))
    assert np.array_equal(h["n_contrib"][o["fragile"] == 0], o["n_contrib"][o["fragile"] == 0])


@pytest.mark.parametrize("split", ["split", "whole"])
def test_deep_and_wide(split):
    _need_gpu()
    from diff_gaussian_rasterization import _C
    scene, cam, D = gr.heavy_scene()
    o, h, dpix = _check_twice(scene, cam, D, f"heavy/{split}", debug=_C.DEBUG_NO_SPLIT if split == "whole" else False)
    lens = h["ranges"][:, 1].astype(np.int64) - h["ranges"][:, 0]
    assert lens.max() >= 4 * 512, f"longest list {lens.max()}: no tile deep enough for depth segments"
    if split == "split":
        # the splits happened: the band waves leave the image's bits alone, a depth segment starts its accum_rec from the forward's
        # colour sums and leaves the blend sums at other bits than the whole walk
        w = util.hip_forward_backward(scene, cam, D, dpix, debug=_C.DEBUG_NO_SPLIT)
        _same_bits(h["color"], w["color"], "color split / whole")
        assert any(h["raw_grads"][k].tobytes() != w["raw_grads"][k].tobytes() for k in gr.TENSORS), "no tile was walked in depth segments"
