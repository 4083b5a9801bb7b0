// gaussian_backward_tail.inc -- the tail of gsr_gaussian_backward_kernel's branch of the visible lanes: the SH, covariance and
// leaf-activation backward.  Included twice by gaussian_backward.hip, as text: where the statements always stood, and, in the CAM
// kernels, behind the whole-wave sums of the view and projection rows, for which the branch has to be closed and reopened (a lambda
// in its place changed the register allocation of the other kernels).
		if (a.shs) {
			if (sh_via_lds) {
				// dL_dsh = basis x dL/dRGB: kept as its two factors until the block store below
				gsr_sh_backward<CAM>(a.D, M, mean, a.cam_pos, ddir9, clamp_bits, dcolor, dmean3D, nullptr, false, dRGB, basis_keep, cam_dm);
				if (!skip_dsh && LEAF) {
					const int used_sh = (a.D + 1) * (a.D + 1);
					float o[48];
#pragma unroll
					for (int e = 0; e < 48; e++) o[e] = (e / 3 < used_sh) ? basis_keep[e / 3] * dRGB[e % 3] : 0.f;
					gsr_sh_lin_row_put(reinterpret_cast<float*>(s_sh[wave]), lane, o);
				}
			} else if (LEAF) {
				const int used = (a.D + 1) * (a.D + 1);
				float basis[16];
				gsr_sh_backward<CAM>(a.D, used, mean, a.cam_pos, ddir9, clamp_bits, dcolor, dmean3D, nullptr, false, dRGB, basis, cam_dm);
#pragma unroll
				for (int e = 0; e < 48; e++) dsh_local[e] = (e / 3 < used) ? basis[e / 3] * dRGB[e % 3] : 0.f;
			} else {
				gsr_sh_backward<CAM>(a.D, M, mean, a.cam_pos, ddir9, clamp_bits, dcolor, dmean3D, dsh_global, !skip_dsh, dRGB, nullptr, cam_dm);
			}
		}
		if (a.scales)
			gsr_cov3d_backward(sc, a.scale_modifier, q, dcov, dscale, drot);
		if (LEAF) {
			// exp backward: grad * result;  sigmoid backward: grad * ((1 - y) * y)
			dscale[0] *= sc[0]; dscale[1] *= sc[1]; dscale[2] *= sc[2];
			const float o = leaf_opacity;
			dop = dop * ((1.0f - o) * o);
			// F.normalize backward: y = x / d, d = clamp_min(||x||, 1e-12)
			float gd = 0.f;
#pragma unroll
			for (int k = 0; k < 4; k++) gd += -drot[k] * q_raw[k] / (q_den * q_den);
			const float r = (q_den > 1e-12f) ? gd / q_den : 0.f;
#pragma unroll
			for (int k = 0; k < 4; k++) drot[k] = drot[k] / q_den + q_raw[k] * r;
		}
