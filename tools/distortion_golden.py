#!/usr/bin/env python3
"""Writes tests/golden/distortion_B_camera_terms.npz: the float64 per-Gaussian camera terms of scene B of tests/test_distortion_gpu.py
(3000 Gaussians at 120 x 90, mode "depth", the test's own seeds) for the loss sum(image dpix) + sum(distortion g) on the pixels the
oracle does not call fragile, reduced to what test_variant_camera_grads scales its bar with -- sum_g t_g, sum_g |t_g| and the
float32 helper's distance d32 per camera tensor (tests/torch_splat_dist.camera_terms; the rule of tests/test_camera_grads_gpu.py).
CPU only, about a minute and several GB: too slow for the suite, so the numbers are kept as a fixture.  Run from the repository
root after changing scene B or its seeds."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting_cc-comments_amd"), os.path.join(ROOT, "tests")]
import __graft_entry__  # noqa: E402,F401
import gsr_scene  # noqa: E402
import torch_splat_dist  # noqa: E402
import util  # noqa: E402

P, MU, D, SEED, W, H, UP_SEED, MARGIN = 3000, -3.0, 1, 21, 120, 90, 47, 1e-3


def main():
    scene, cam = gsr_scene.make_scene(P, MU, sh_degree=D, seed=SEED), gsr_scene.make_camera(W, H)
    o = util.oracle_forward(scene, cam, D, margin=MARGIN)
    ok = torch.from_numpy((o["fragile"] == 0).reshape(H, W))
    g = torch.Generator().manual_seed(UP_SEED)
    dpix, gd = torch.randn(3, H, W, generator=g) * ok, torch.randn(1, H, W, generator=g) * ok
    inputs = dict(means3D=scene.means3D, opacities=scene.opacities, shs=scene.shs, scales=scene.scales, rotations=scene.rotations,
                  V=cam.world_view_transform, PM=cam.full_proj_transform, campos=cam.camera_center)
    total, abs_total, d32 = torch_splat_dist.camera_terms(o, inputs, "depth", (dpix, None, None, gd))
    out = os.path.join(ROOT, "tests", "golden", "distortion_B_camera_terms.npz")
    np.savez(out, scene=np.array([P, D, SEED, W, H, UP_SEED]), margin=np.float64(MARGIN), ok=ok.numpy(),
             **{f"total_{k}": total[k].numpy() for k in total}, **{f"abs_total_{k}": abs_total[k].numpy() for k in total},
             **{f"d32_{k}": np.float64(d32[k]) for k in total})
    for k in total:
        print(k, "max |total|", float(total[k].abs().max()), "max sum |t_g|", float(abs_total[k].max()), "d32", d32[k])
    print("fragile share", float((~ok).float().mean()))
    print("wrote", out)


if __name__ == "__main__":
    main()
