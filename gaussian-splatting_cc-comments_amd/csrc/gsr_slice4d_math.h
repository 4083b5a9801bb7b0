// gsr_slice4d_math.h -- the per-Gaussian arithmetic of the 4D time slice (include/gsr_slice4d.h), in double from the float32 leaves.
// Plain C++ with every loop bound a constant: under hipcc the functions are inlined into the two kernels of slice4d.hip and, fully
// unrolled, index their 4 x 4 arrays with constants only, so that nothing lives in scratch memory; a host compiler takes the same text
// (the CPU check of the hand-derived chain needs no device).
#ifndef GSR_SLICE4D_MATH_H_INCLUDED
#define GSR_SLICE4D_MATH_H_INCLUDED
#include <math.h>

#if defined(__HIPCC__)
#define GSR_S4D_FN __host__ __device__ __forceinline__
#define GSR_S4D_UNROLL _Pragma("unroll")
#else
#define GSR_S4D_FN static inline
#define GSR_S4D_UNROLL
#endif

struct GsrS4dLeaves {
	float xyz[3], t, ls[4] /* x y z t */, l[4], r[4], o;
};

// what forward and backward share: the unit quaternions with the reciprocal norms, R = L(l^) M(r^), w_k = (m exp(ls_k))^2,
// Sigma_tt, u = Sigma[:3, 3], Delta, g, and sigmoid(o) with sigmoid(o) sigmoid(-o) from one exponential
struct GsrS4dEval {
	double lh[4], rh[4], iln, irn;
	double R[4][4], w[4];
	double stt, u[3], delta, g, sig, dsig;
};

GSR_S4D_FN void gsr_s4d_left(const double q[4], double L[4][4])
{
	const double a = q[0], b = q[1], c = q[2], d = q[3];
	L[0][0] = a;  L[0][1] = -d; L[0][2] = c;  L[0][3] = b;
	L[1][0] = d;  L[1][1] = a;  L[1][2] = -b; L[1][3] = c;
	L[2][0] = -c; L[2][1] = b;  L[2][2] = a;  L[2][3] = d;
	L[3][0] = -b; L[3][1] = -c; L[3][2] = -d; L[3][3] = a;
}

GSR_S4D_FN void gsr_s4d_right(const double q[4], double M[4][4])
{
	const double p = q[0], q1 = q[1], r = q[2], s = q[3];
	M[0][0] = p;   M[0][1] = -s; M[0][2] = r;   M[0][3] = -q1;
	M[1][0] = s;   M[1][1] = p;  M[1][2] = -q1; M[1][3] = -r;
	M[2][0] = -r;  M[2][1] = q1; M[2][2] = p;   M[2][3] = -s;
	M[3][0] = q1;  M[3][1] = r;  M[3][2] = s;   M[3][3] = p;
}

GSR_S4D_FN void gsr_s4d_eval(const GsrS4dLeaves& in, double time, double modifier, GsrS4dEval& v)
{
	double nl = 0.0, nr = 0.0;
	GSR_S4D_UNROLL
	for (int k = 0; k < 4; k++) {
		nl += (double)in.l[k] * (double)in.l[k];
		nr += (double)in.r[k] * (double)in.r[k];
	}
	v.iln = 1.0 / sqrt(nl);
	v.irn = 1.0 / sqrt(nr);
	GSR_S4D_UNROLL
	for (int k = 0; k < 4; k++) {
		v.lh[k] = (double)in.l[k] * v.iln;
		v.rh[k] = (double)in.r[k] * v.irn;
		const double s = modifier * exp((double)in.ls[k]);
		v.w[k] = s * s;
	}
	double L[4][4], M[4][4];
	gsr_s4d_left(v.lh, L);
	gsr_s4d_right(v.rh, M);
	GSR_S4D_UNROLL
	for (int i = 0; i < 4; i++) {
		GSR_S4D_UNROLL
		for (int j = 0; j < 4; j++) v.R[i][j] = L[i][0] * M[0][j] + L[i][1] * M[1][j] + L[i][2] * M[2][j] + L[i][3] * M[3][j];
	}
	v.stt = 0.0;
	GSR_S4D_UNROLL
	for (int k = 0; k < 4; k++) v.stt += v.R[3][k] * v.R[3][k] * v.w[k];
	GSR_S4D_UNROLL
	for (int i = 0; i < 3; i++) {
		v.u[i] = 0.0;
		GSR_S4D_UNROLL
		for (int k = 0; k < 4; k++) v.u[i] += v.R[i][k] * v.R[3][k] * v.w[k];
	}
	v.delta = time - (double)in.t;
	v.g = exp(-0.5 * v.delta * v.delta / v.stt);
	const double e = exp(-fabs((double)in.o));   // <= 1
	const double big = 1.0 / (1.0 + e), small = e * big;
	v.sig = in.o >= 0.0f ? big : small;
	v.dsig = big * small;
}

// Sigma[i][j] of the spatial block, i <= j < 3
GSR_S4D_FN double gsr_s4d_sigma11(const GsrS4dEval& v, int i, int j)
{
	return v.R[i][0] * v.R[j][0] * v.w[0] + v.R[i][1] * v.R[j][1] * v.w[1] + v.R[i][2] * v.R[j][2] * v.w[2] + v.R[i][3] * v.R[j][3] * v.w[3];
}

struct GsrS4dGrads {
	double xyz[3], t, ls[4], l[4], r[4], o;
};

// The chain of an unmasked row.  gm, gv [3], gc [6] (w.r.t. the six stored values), go: the incoming gradients, zeros where absent.
// With G the symmetric 3 x 3 matrix of gc (off-diagonal entries halved), gvt = gv + gm Delta and D the symmetric 4 x 4 matrix of
// dL/dSigma:
//   dL/du       = (gvt - 2 G u) / Sigma_tt
//   dL/dSigma_tt= (u^T G u - gvt . u + go sigmoid g Delta^2 / 2) / Sigma_tt^2
//   D           = [[G, dL/du / 2], [dL/du^T / 2, dL/dSigma_tt]]
//   dL/dw_k     = (R^T D R)_kk,  dL/dlog-scale_k = 2 w_k dL/dw_k,  dL/dR = 2 D R diag(w)
//   dL/dL       = dL/dR M^T,  dL/dM = L^T dL/dR, folded onto the four components each matrix is linear in, then through q / |q|
GSR_S4D_FN void gsr_s4d_chain(const GsrS4dEval& v, const double gm[3], const double gc[6], double go, const double gv[3], GsrS4dGrads& out)
{
	double D[4][4];
	D[0][0] = gc[0]; D[1][1] = gc[3]; D[2][2] = gc[5];
	D[0][1] = D[1][0] = 0.5 * gc[1];
	D[0][2] = D[2][0] = 0.5 * gc[2];
	D[1][2] = D[2][1] = 0.5 * gc[4];
	const double istt = 1.0 / v.stt;
	const double through_g = go * v.sig * v.g;
	double gvt[3], Gu[3], uGu = 0.0, gvtu = 0.0, gmu = 0.0;
	GSR_S4D_UNROLL
	for (int i = 0; i < 3; i++) {
		gvt[i] = gv[i] + gm[i] * v.delta;
		Gu[i] = D[i][0] * v.u[0] + D[i][1] * v.u[1] + D[i][2] * v.u[2];
		uGu += v.u[i] * Gu[i];
		gvtu += gvt[i] * v.u[i];
		gmu += gm[i] * v.u[i];
	}
	GSR_S4D_UNROLL
	for (int i = 0; i < 3; i++) D[i][3] = D[3][i] = 0.5 * (gvt[i] - 2.0 * Gu[i]) * istt;
	D[3][3] = (uGu - gvtu + through_g * 0.5 * v.delta * v.delta) * istt * istt;

	double GR[4][4];   // D R first, then 2 (D R) diag(w)
	GSR_S4D_UNROLL
	for (int i = 0; i < 4; i++) {
		GSR_S4D_UNROLL
		for (int k = 0; k < 4; k++) GR[i][k] = D[i][0] * v.R[0][k] + D[i][1] * v.R[1][k] + D[i][2] * v.R[2][k] + D[i][3] * v.R[3][k];
	}
	GSR_S4D_UNROLL
	for (int k = 0; k < 4; k++) {
		const double dw = v.R[0][k] * GR[0][k] + v.R[1][k] * GR[1][k] + v.R[2][k] * GR[2][k] + v.R[3][k] * GR[3][k];
		out.ls[k] = 2.0 * v.w[k] * dw;
		GSR_S4D_UNROLL
		for (int i = 0; i < 4; i++) GR[i][k] *= 2.0 * v.w[k];
	}
	double L[4][4], M[4][4], X[4][4], Y[4][4];
	gsr_s4d_left(v.lh, L);
	gsr_s4d_right(v.rh, M);
	GSR_S4D_UNROLL
	for (int i = 0; i < 4; i++) {
		GSR_S4D_UNROLL
		for (int j = 0; j < 4; j++) {
			X[i][j] = GR[i][0] * M[j][0] + GR[i][1] * M[j][1] + GR[i][2] * M[j][2] + GR[i][3] * M[j][3];
			Y[i][j] = L[0][i] * GR[0][j] + L[1][i] * GR[1][j] + L[2][i] * GR[2][j] + L[3][i] * GR[3][j];
		}
	}
	double dl[4], dr[4];
	dl[0] = X[0][0] + X[1][1] + X[2][2] + X[3][3];
	dl[1] = X[0][3] - X[1][2] + X[2][1] - X[3][0];
	dl[2] = X[0][2] + X[1][3] - X[2][0] - X[3][1];
	dl[3] = -X[0][1] + X[1][0] + X[2][3] - X[3][2];
	dr[0] = Y[0][0] + Y[1][1] + Y[2][2] + Y[3][3];
	dr[1] = -Y[0][3] - Y[1][2] + Y[2][1] + Y[3][0];
	dr[2] = Y[0][2] - Y[1][3] - Y[2][0] + Y[3][1];
	dr[3] = -Y[0][1] + Y[1][0] - Y[2][3] + Y[3][2];
	const double pl = v.lh[0] * dl[0] + v.lh[1] * dl[1] + v.lh[2] * dl[2] + v.lh[3] * dl[3];
	const double pr = v.rh[0] * dr[0] + v.rh[1] * dr[1] + v.rh[2] * dr[2] + v.rh[3] * dr[3];
	GSR_S4D_UNROLL
	for (int k = 0; k < 4; k++) {
		out.l[k] = (dl[k] - v.lh[k] * pl) * v.iln;
		out.r[k] = (dr[k] - v.rh[k] * pr) * v.irn;
	}
	GSR_S4D_UNROLL
	for (int i = 0; i < 3; i++) out.xyz[i] = gm[i];
	out.t = (through_g * v.delta - gmu) * istt;
	out.o = go * v.g * v.dsig;
}
#endif /* GSR_SLICE4D_MATH_H_INCLUDED */
