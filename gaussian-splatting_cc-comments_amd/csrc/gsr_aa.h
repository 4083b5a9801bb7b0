// gsr_aa.h -- the opacity compensation of the anti-aliased path (include/gsr_aa.h): the screen-space filter of Mip-Splatting.
//
// The projected covariance Sigma = [[a, b], [b, c]] is always dilated by h = 0.3 px^2 on each diagonal entry (gsr_cov2d), which widens a
// sub-pixel Gaussian to a 0.3-px^2 blob.  At full opacity its footprint integral then grows by sqrt(det(Sigma + hI) / det Sigma).  The
// anti-aliased path scales the opacity by the inverse of that factor:
//     N = a c - b^2,  Dh = (a + h)(c + h) - b^2 (the `det` of the preprocess kernel),  rho = sqrt(max(2.5e-5, N / Dh))
// and the splat record carries opacity * rho, so the blend and the tile trim see the compensated value.  The derivatives are taken at the
// UNDILATED entries; d rho / d r = 1 / (2 rho) with r = N / Dh, zero where the floor holds (r <= 2.5e-5):
//     dr/da = h (c^2 + h c + b^2) / Dh^2,   dr/dc = h (a^2 + h a + b^2) / Dh^2,   dr/db = -2 h b (a + c + h) / Dh^2
// Host and device: tests/test_antialias_cpu.py compiles it for the host.  Both callers are built -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define GSR_AA_DILATION 0.3f     // h: the dilation of gsr_cov2d
#define GSR_AA_FLOOR 2.5e-5f     // the floor of N / Dh (rho >= 0.005)

// rho of the undilated entries (a, b, c); the dilated determinant is formed as gsr_cov2d's (a + 0.3f) and the preprocess kernel's det
__host__ __device__ __forceinline__ float gsr_aa_rho(float a, float b, float c)
{
	const float h = GSR_AA_DILATION;
	const float N = a * c - b * b;
	const float Dh = (a + h) * (c + h) - b * b;
	return sqrtf(fmaxf(GSR_AA_FLOOR, N / Dh));
}

// rho and its partials d rho / d{a, b, c} at the undilated entries
struct GsrAAGrad {
	float rho, drho_da, drho_db, drho_dc;
};
__host__ __device__ __forceinline__ GsrAAGrad gsr_aa_rho_grad(float a, float b, float c)
{
	const float h = GSR_AA_DILATION;
	const float N = a * c - b * b;
	const float Dh = (a + h) * (c + h) - b * b;
	const float r = N / Dh;
	GsrAAGrad o;
	o.rho = sqrtf(fmaxf(GSR_AA_FLOOR, r));
	const float g = r > GSR_AA_FLOOR ? 0.5f / o.rho : 0.f;   // d rho / d r
	o.drho_da = g * (h * (c * c + h * c + b * b) / Dh / Dh);   // (over Dh twice: Dh^2 would overflow first)
	o.drho_dc = g * (h * (a * a + h * a + b * b) / Dh / Dh);
	o.drho_db = g * (-2.f * h * b * (a + c + h) / Dh / Dh);
	return o;
}
