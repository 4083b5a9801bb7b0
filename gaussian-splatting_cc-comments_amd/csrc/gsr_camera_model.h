// gsr_camera_model.h -- projection, EWA Jacobian and their backward for the camera models of include/gsr_camera_model.h.
//
// Shared by gsr_preprocess_kernel and gsr_gaussian_backward_kernel (their CM instantiations), the way both call gsr_cov2d for the
// core camera: the backward recomputes the forward's values with the same expressions, bit for bit.  Compiled with -ffp-contract=off
// like everything that decides radii and rectangles.  The model is a wave-uniform run-time switch (a kernel argument).
#pragma once
#include "gsr_device.h"
#include "../../include/gsr_camera_model.h"

// What the CM kernels receive behind their usual arguments: a struct of its own, so that the other instantiations keep their argument
// layout and their instruction stream (as GsrGaussianBackwardCam does).  fx and fy travel in the usual focal_x, focal_y.
template <typename Base>
struct GsrWithCameraModel : Base {
	int cm_model;        // GSR_CAMERA_*
	float cm_cx, cm_cy;  // principal point, pixels (corner origin)
};

// ---- equidistant fisheye ------------------------------------------------------------------------------------------------------------
// With r2 = x^2 + y^2, d2 = r2 + z^2, q = r2 / z^2, theta = atan2(r, z):
//   s   = theta / r                          u = fx s x + cx - 0.5
//   A   = (z / d2 - s) / r2                  ds/dx = x A, ds/dy = y A, ds/dz = -1 / d2
//   Ar2 = dA/d(r2) = (-z / d2^2 - 1.5 A) / r2,   dA/dz = 2 / d2^2 (exactly)
// s is 0/0 on the axis, A cancels like eps / q and Ar2 like eps / q^2.  Below GSR_CM_SERIES_Q all three come from their Taylor series
//   s   = (1/z)   sum_{k>=0} (-1)^k q^k / (2k+1)
//   A   = (1/z^3) sum_{k>=1} (-1)^k 2k / (2k+1) q^(k-1)
//   Ar2 = (1/z^5) sum_{k>=2} (-1)^k 2k (k-1) / (2k+1) q^(k-2)
// with ten terms each (eleven for s, so that A's series is the derivative of s's term by term): at q = 0.1 the first omitted terms are
// 4e-13, 1e-10 and 1e-9 of the leading ones, far below fp32 rounding, while
// the closed forms are at their best there (relative cancellation errors about 6e-7 for A and 6e-6 for Ar2).  q = 0.1 is r / z = 0.316,
// theta = 17.5 degrees.
#define GSR_CM_SERIES_Q 0.1f
#define GSR_CM_SERIES_TERMS 10

struct GsrFisheye { float s, A, Ar2, id2; };   // id2 = 1 / d2

__device__ __forceinline__ GsrFisheye gsr_fisheye_terms(float x, float y, float z)
{
	GsrFisheye f;
	const float r2 = x * x + y * y, z2 = z * z;
	const float d2 = r2 + z2;
	f.id2 = 1.0f / d2;
	const float q = r2 / z2;
	if (q < GSR_CM_SERIES_Q) {
		float ps = (GSR_CM_SERIES_TERMS & 1) ? -1.f / (float)(2 * GSR_CM_SERIES_TERMS + 1) : 1.f / (float)(2 * GSR_CM_SERIES_TERMS + 1);
		float pa = 0.f, pr = 0.f;   // (s carries one term more: its derivative is then A's series term by term)
#pragma unroll
		for (int k = GSR_CM_SERIES_TERMS - 1; k >= 0; k--) {   // Horner, highest power first; the coefficients fold to constants
			const float sign = (k & 1) ? -1.f : 1.f;
			const int ka = k + 1, kr = k + 2;                   // the series' own k of the term in q^k
			ps = ps * q + sign / (float)(2 * k + 1);
			pa = pa * q - sign * (float)(2 * ka) / (float)(2 * ka + 1);
			pr = pr * q + sign * (float)(2 * kr * (kr - 1)) / (float)(2 * kr + 1);
		}
		const float iz = 1.0f / z;
		const float iz3 = iz / z2;
		f.s = ps * iz;
		f.A = pa * iz3;
		f.Ar2 = pr * (iz3 / z2);
	} else {
		const float r = sqrtf(r2);
		f.s = atan2f(r, z) / r;
		f.A = (z * f.id2 - f.s) / r2;
		f.Ar2 = (-(z * f.id2 * f.id2) - 1.5f * f.A) / r2;
	}
	return f;
}

// the pinhole's guard band along one axis: t.x / t.z is clamped to [lo, hi] inside the Jacobian (the core camera: +-1.3 tan_fov)
__device__ __forceinline__ void gsr_cm_band(float f, float c, int S, float& lo, float& hi)
{
	const float margin = 0.3f * (float)S / (2.0f * f);
	lo = -(c / f + margin);
	hi = ((float)S - c) / f + margin;
}

struct GsrCmExtra {
	GsrVec3 traw;                    // the view-space mean itself (GsrCov2D::t holds the clamped one, as for the core camera)
	float lox, hix, loy, hiy;        // pinhole: the guard band
	GsrFisheye f;                    // fisheye: the terms the Jacobian was formed from, for gsr_cm_backward
};

// gsr_cov2d for a camera model -> the same GsrCov2D (limx / limy unused), the pixel-index mean (u, v) and GsrCmExtra
__device__ __forceinline__ void gsr_cm_cov2d(const GsrVec3& mean, int model, float fx, float fy, float cx, float cy, int W, int H,
                                             const float* cov3D, const float* vm, GsrCov2D& o, GsrCmExtra& e, float& u, float& v)
{
	GsrVec3 t = gsr_transform_point_4x3(mean, vm);
	e.traw = t;
	GsrMat3 J;
	if (model == GSR_CAMERA_FISHEYE) {
		const GsrFisheye f = gsr_fisheye_terms(t.x, t.y, t.z);
		e.f = f;
		u = fx * (f.s * t.x) + (cx - 0.5f);
		v = fy * (f.s * t.y) + (cy - 0.5f);
		const float xyA = t.x * t.y * f.A;
		J.m[0][0] = fx * (f.s + t.x * t.x * f.A); J.m[0][1] = fx * xyA; J.m[0][2] = -(fx * t.x) * f.id2;
		J.m[1][0] = fy * xyA; J.m[1][1] = fy * (f.s + t.y * t.y * f.A); J.m[1][2] = -(fy * t.y) * f.id2;
		o.txtz = 0.f; o.tytz = 0.f;
		e.lox = e.hix = e.loy = e.hiy = 0.f;
	} else {
		e.f.s = e.f.A = e.f.Ar2 = e.f.id2 = 0.f;
		gsr_cm_band(fx, cx, W, e.lox, e.hix);
		gsr_cm_band(fy, cy, H, e.loy, e.hiy);
		o.txtz = t.x / t.z;
		o.tytz = t.y / t.z;
		u = fx * o.txtz + (cx - 0.5f);
		v = fy * o.tytz + (cy - 0.5f);
		t.x = fminf(e.hix, fmaxf(e.lox, o.txtz)) * t.z;
		t.y = fminf(e.hiy, fmaxf(e.loy, o.tytz)) * t.z;
		J.m[0][0] = fx / t.z; J.m[0][1] = 0.0f; J.m[0][2] = -(fx * t.x) / (t.z * t.z);
		J.m[1][0] = 0.0f; J.m[1][1] = fy / t.z; J.m[1][2] = -(fy * t.y) / (t.z * t.z);
	}
	o.limx = 0.f; o.limy = 0.f;
	o.t = t;
	J.m[2][0] = 0.f; J.m[2][1] = 0.f; J.m[2][2] = 0.f;
	o.W.m[0][0] = vm[0]; o.W.m[0][1] = vm[4]; o.W.m[0][2] = vm[8];
	o.W.m[1][0] = vm[1]; o.W.m[1][1] = vm[5]; o.W.m[1][2] = vm[9];
	o.W.m[2][0] = vm[2]; o.W.m[2][1] = vm[6]; o.W.m[2][2] = vm[10];
	o.T = gsr_mat3_mul(o.W, J);
	o.Vrk.m[0][0] = cov3D[0]; o.Vrk.m[0][1] = cov3D[1]; o.Vrk.m[0][2] = cov3D[2];
	o.Vrk.m[1][0] = cov3D[1]; o.Vrk.m[1][1] = cov3D[3]; o.Vrk.m[1][2] = cov3D[4];
	o.Vrk.m[2][0] = cov3D[2]; o.Vrk.m[2][1] = cov3D[4]; o.Vrk.m[2][2] = cov3D[5];
	GsrMat3 cov = gsr_mat3_mul(gsr_mat3_mul(gsr_mat3_transpose(o.T), gsr_mat3_transpose(o.Vrk)), o.T);
	o.a0 = cov.m[0][0];
	o.c0 = cov.m[1][1];
	o.a = cov.m[0][0] + 0.3f;
	o.b = cov.m[0][1];
	o.c = cov.m[1][1] + 0.3f;
}

// dL/dt (view space) from dL/dJ (dJ[3 i + k] = dL / d(d pixel_i / d t_k)) and dL/d(u, v) in pixels.
//   pinhole: the core camera's expressions with fx, fy and the asymmetric band (a clamped coordinate is a constant), plus J^T (du, dv)
//            of the unclamped projection in place of the projection matrix's chain
//   fisheye: the second derivatives of the projection.  With j00 = s + x^2 A, j01 = x y A, j02 = -x / d2, j11 = s + y^2 A,
//            j12 = -y / d2 (J = diag(fx, fy) j, J10 = fy j01) and D = 2 / d2^2:
//              d j00 = (3 x A + 2 x^3 Ar2,  y A + 2 x^2 y Ar2,  -1/d2 + x^2 D)
//              d j01 = (y A + 2 x^2 y Ar2,  x A + 2 x y^2 Ar2,  x y D)
//              d j02 = (-1/d2 + x^2 D,      x y D,              x z D)
//              d j11 = (x A + 2 x y^2 Ar2,  3 y A + 2 y^3 Ar2,  -1/d2 + y^2 D)
//              d j12 = (x y D,              -1/d2 + y^2 D,      y z D)
__device__ __forceinline__ void gsr_cm_backward(int model, float fx, float fy, const GsrCov2D& c2, const GsrCmExtra& e,
                                                const float* dJ, float du, float dv, float* dt)
{
	const float x = e.traw.x, y = e.traw.y, z = e.traw.z;
	if (model == GSR_CAMERA_FISHEYE) {
		const GsrFisheye& f = e.f;   // as gsr_cm_cov2d evaluated them
		const float g00 = fx * dJ[0], g01 = fx * dJ[1] + fy * dJ[3], g02 = fx * dJ[2], g11 = fy * dJ[4], g12 = fy * dJ[5];
		const float D = 2.0f * f.id2 * f.id2;
		const float xA = x * f.A, yA = y * f.A;
		const float x2 = 2.0f * x * f.Ar2, y2 = 2.0f * y * f.Ar2;       // dA/dx, dA/dy
		const float xx = x * x, yy = y * y, xy = x * y;
		const float b = -f.id2;
		const float j00x = 3.0f * xA + xx * x2, j00y = yA + xx * y2, j00z = b + xx * D;
		const float j01x = yA + xy * x2, j01y = xA + xy * y2, j01z = xy * D;
		const float j02x = b + xx * D, j02y = xy * D, j02z = x * z * D;
		const float j11x = xA + yy * x2, j11y = 3.0f * yA + yy * y2, j11z = b + yy * D;
		const float j12x = xy * D, j12y = b + yy * D, j12z = y * z * D;
		// J^T (du, dv): the Jacobian's own entries
		const float J00 = fx * (f.s + xx * f.A), J01 = fx * (xy * f.A), J02 = -(fx * x) * f.id2;
		const float J10 = fy * (xy * f.A), J11 = fy * (f.s + yy * f.A), J12 = -(fy * y) * f.id2;
		dt[0] = g00 * j00x + g01 * j01x + g02 * j02x + g11 * j11x + g12 * j12x + (J00 * du + J10 * dv);
		dt[1] = g00 * j00y + g01 * j01y + g02 * j02y + g11 * j11y + g12 * j12y + (J01 * du + J11 * dv);
		dt[2] = g00 * j00z + g01 * j01z + g02 * j02z + g11 * j11z + g12 * j12z + (J02 * du + J12 * dv);
	} else {
		const float x_grad_mul = (c2.txtz < e.lox || c2.txtz > e.hix) ? 0.f : 1.f;
		const float y_grad_mul = (c2.tytz < e.loy || c2.tytz > e.hiy) ? 0.f : 1.f;
		const float tz = 1.f / z;
		const float tz2 = tz * tz;
		const float tz3 = tz2 * tz;
		dt[0] = x_grad_mul * -fx * tz2 * dJ[2] + fx * tz * du;
		dt[1] = y_grad_mul * -fy * tz2 * dJ[5] + fy * tz * dv;
		dt[2] = -fx * tz2 * dJ[0] - fy * tz2 * dJ[4] + (2 * fx * c2.t.x) * tz3 * dJ[2] + (2 * fy * c2.t.y) * tz3 * dJ[5] -
		        ((fx * x) * tz2 * du + (fy * y) * tz2 * dv);
	}
}

// ---- camera gradients under a model (include/gsr_cam_cm.h) ---------------------------------------------------------------------------
// J[3 i + k] = d pixel_i / d t_k exactly as gsr_cm_cov2d formed it (the same expressions on the same values: the same bits), for the
// rotation half of T = W J: dL/dW[i][k] = J[0][i] dL/dT0k + J[1][i] dL/dT1k.  Pinhole: J01 = J10 = 0, J02 / J12 from the clamped coordinate.
__device__ __forceinline__ void gsr_cm_jacobian(int model, float fx, float fy, const GsrCov2D& c2, const GsrCmExtra& e, float* J)
{
	if (model == GSR_CAMERA_FISHEYE) {
		const GsrFisheye& f = e.f;
		const float x = e.traw.x, y = e.traw.y;
		const float xyA = x * y * f.A;
		J[0] = fx * (f.s + x * x * f.A); J[1] = fx * xyA; J[2] = -(fx * x) * f.id2;
		J[3] = fy * xyA; J[4] = fy * (f.s + y * y * f.A); J[5] = -(fy * y) * f.id2;
	} else {
		const GsrVec3 t = c2.t;   // x and y clamped to the guard band
		J[0] = fx / t.z; J[1] = 0.0f; J[2] = -(fx * t.x) / (t.z * t.z);
		J[3] = 0.0f; J[4] = fy / t.z; J[5] = -(fy * t.y) / (t.z * t.z);
	}
}

// dL/d(fx, fy, cx, cy) of one Gaussian from dL/dJ (dJ[3 i + k], as for gsr_cm_backward) and dL/d(u, v) in pixels.  Every entry of J's
// row 0 is fx times a function of t alone, and u = fx (...) + cx - 0.5, so nothing is divided by fx:
//   pinhole: dL/dfx = dJ00 / z - dJ02 x_c / z^2 + du x / z   (x_c the clamped coordinate, a constant; x the raw one; the band's limits
//            carry no gradient with respect to fx and cx)
//   fisheye: dL/dfx = dJ00 (s + x^2 A) + dJ01 x y A - dJ02 x / d2 + du s x   with the s, A, 1 / d2 gsr_cm_cov2d evaluated (the series
//            near the axis serves here too)
// fy likewise with row 1; dL/dcx = du, dL/dcy = dv.
__device__ __forceinline__ void gsr_cm_intrinsics_grad(int model, const GsrCov2D& c2, const GsrCmExtra& e, const float* dJ, float du,
                                                       float dv, float* dk)
{
	const float x = e.traw.x, y = e.traw.y, z = e.traw.z;
	if (model == GSR_CAMERA_FISHEYE) {
		const GsrFisheye& f = e.f;
		const float xyA = x * y * f.A;
		dk[0] = dJ[0] * (f.s + x * x * f.A) + dJ[1] * xyA - dJ[2] * x * f.id2 + du * (f.s * x);
		dk[1] = dJ[3] * xyA + dJ[4] * (f.s + y * y * f.A) - dJ[5] * y * f.id2 + dv * (f.s * y);
	} else {
		const float tz = 1.f / z;
		const float tz2 = tz * tz;
		dk[0] = dJ[0] * tz - dJ[2] * c2.t.x * tz2 + du * (x * tz);
		dk[1] = dJ[4] * tz - dJ[5] * c2.t.y * tz2 + dv * (y * tz);
	}
	dk[2] = du;
	dk[3] = dv;
}
