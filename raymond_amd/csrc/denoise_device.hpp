// The denoise filters' per-pixel arithmetic, each quantity of include/raymond_hip.h once: device code for denoise.hip, denoise_dual.hip,
// denoise_atrous.hip and denoise_atrous_dual.hip, no kernels and no host functions.  The filter kernels (denoise_kernel, denoise_dual_kernel,
// atrous_level_kernel, atrous_dual_level_kernel) call the scalar functions and dual_combine / dual_merged only: a helper that carries their
// loops or arrays changes their registers.  The one-pass kernels share whole pixels, so a region form gives the whole-frame form's bytes by construction.
#pragma once
#include <hip/hip_runtime.h>

#include "launch.hpp"

namespace rmd {

// term_c of two pixels' means and variances of the mean
__device__ inline double denoise_term(double ua, double ub, double va, double vb, double k2, double alpha) {
	const double du = ua - ub;
	return (du * du - alpha * (va + __builtin_fmin(va, vb))) / (kDenoiseEps + k2 * (va + vb));
}

// H5 = {1/16, 1/4, 3/8, 1/4, 1/16} at i + 2, as selects: a table indexed by the loop counters would live in memory
__device__ inline double atrous_h5(int i) { return i == 0 ? 0.375 : (i == 1 || i == -1 ? 0.25 : 0.0625); }

// One channel's mean u = s / n and variance of the mean v = max(0, (q - s*u) / (n - 1)) / n from its sum s, sum of squares q and nd = (double)n, as
// IEEE gives them for every n
__device__ inline void denoise_moments(double s, double q, double nd, double &u, double &v) {
	u = s / nd;
	double t = (q - s * u) / (nd - 1.0);
	if (t < 0.0) t = 0.0;
	v = t / nd;
}
// ... and the finiteness a valid pixel needs of every s and q
__device__ inline bool denoise_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }

// max(tau * s_pj, g_pj), s = 1 but for the depth (the last channel), where it is f_pj^2
__device__ inline double feature_scale(double fp, double gp, int j, double tau) {
	const double a = tau * (j < kDenoiseFeat - 1 ? 1.0 : fp * fp);
	return a > gp ? a : gp;
}
// The denominator of Phi_j(p, .): eps + k_f^2 * max(tau * s_pj, g_pj)
__device__ inline double feature_den(double fp, double gp, int j, double kf2, double tau) { return kDenoiseEps + kf2 * feature_scale(fp, gp, j, tau); }
// ... and with the slope's floor m_pj under it (the _slope calls): m replaces the maximum where it is larger (a NaN m is skipped by the comparison)
__device__ inline double feature_den(double fp, double gp, int j, double kf2, double tau, double m) {
	double t = feature_scale(fp, gp, j, tau);
	if (m > t) t = m;
	return kDenoiseEps + kf2 * t;
}
// One axis' share of a feature's local slope at a pixel with the value f: with a_l = f - f_l and a_r = f_r - f, the smaller of a_l*a_l and a_r*a_r when
// both neighbours are present, else 0.0 — a slope that continues on both sides counts, a step (which has a flat side) does not
__device__ inline double feature_slope_axis(double f, double fl, bool has_l, double fr, bool has_r) {
	if (!(has_l && has_r)) return 0.0;
	const double al = f - fl, ar = fr - f;
	const double l2 = al * al, r2 = ar * ar;
	return l2 < r2 ? l2 : r2;
}
// Pixel i = (x, y)'s seven slope floors m_j = s2 * (h_j + v_j), s2 = slope * slope, from the seven planar f (fplanes: feature_planes_pixel's, N doubles each;
// a NaN in plane 0 marks a pixel that is not FEATURE-VALID) into mplanes.  A neighbour is present if it lies inside the frame and is feature-valid; a pixel
// that is not feature-valid itself gets seven zeros (nothing reads them: it has no feature weight)
__device__ inline void feature_slope_pixel(const double *__restrict__ fplanes, size_t i, uint32_t x, uint32_t y, uint32_t W, uint32_t H, size_t N, double s2,
                                           double *__restrict__ mplanes) {
	const double f0 = fplanes[i];
	const bool ok = f0 == f0;
	bool has_l = false, has_r = false, has_u = false, has_d = false;
	if (ok) {
		if (x >= 1u) has_l = fplanes[i - 1] == fplanes[i - 1];
		if (x + 1u < W) has_r = fplanes[i + 1] == fplanes[i + 1];
		if (y >= 1u) has_u = fplanes[i - W] == fplanes[i - W];
		if (y + 1u < H) has_d = fplanes[i + W] == fplanes[i + W];
	}
#pragma unroll
	for (int j = 0; j < kDenoiseFeat; j++) {
		const double *fj = fplanes + (size_t)j * N;
		double m = 0.0;
		if (ok) {
			const double f = j == 0 ? f0 : fj[i];
			const double h = feature_slope_axis(f, has_l ? fj[i - 1] : 0.0, has_l, has_r ? fj[i + 1] : 0.0, has_r);
			const double v = feature_slope_axis(f, has_u ? fj[i - W] : 0.0, has_u, has_d ? fj[i + W] : 0.0, has_d);
			m = s2 * (h + v);
		}
		mplanes[(size_t)j * N + i] = m;
	}
}
// Phi_j(p, q) (a NaN loses the caller's `phi > Df`)
__device__ inline double feature_phi(double fp, double gp, double den, double fq, double gq) {
	const double df = fp - fq;
	return (df * df - (gp + __builtin_fmin(gp, gq))) / den;
}

// Pixel i's three u and v from the interleaved S, Q at count n; true when it is VALID (n >= 2, six finite sums)
__device__ inline bool moments_pixel(const double *__restrict__ S, const double *__restrict__ Q, size_t i, uint32_t n, double u[3], double v[3]) {
	const double nd = (double)n;
	bool valid = n >= 2u;
#pragma unroll
	for (int c = 0; c < 3; c++) {
		const double s = S[i * 3 + c], q = Q[i * 3 + c];
		valid = valid && denoise_finite(s) && denoise_finite(q);
		denoise_moments(s, q, nd, u[c], v[c]);
	}
	return valid;
}

// Pixel i's twelve planes (N doubles each): half h's u in planes 6h + c, its v in 6h + 3 + c.  A pixel that is not DUAL-VALID (both halves valid) gets a
// NaN in the u of channel 0 of BOTH halves, so one test reads "valid" as dual-valid everywhere.  Returns the dual-validity.
__device__ inline bool dual_planes_pixel(const double *__restrict__ SA, const double *__restrict__ QA, const double *__restrict__ SB, const double *__restrict__ QB,
                                         uint32_t na, uint32_t nb, size_t i, size_t N, double *__restrict__ planes) {
	double u[2][3], v[2][3];
	const bool valid_a = moments_pixel(SA, QA, i, na, u[0], v[0]), valid_b = moments_pixel(SB, QB, i, nb, u[1], v[1]);
	const bool dual = valid_a && valid_b;
#pragma unroll
	for (int h = 0; h < 2; h++) {
#pragma unroll
		for (int c = 0; c < 3; c++) {
			planes[(size_t)(6 * h + c) * N + i] = (c == 0 && !dual) ? __builtin_nan("") : u[h][c];
			planes[(size_t)(6 * h + 3 + c) * N + i] = v[h][c];
		}
	}
	return dual;
}

// Pixel i's fourteen feature planes from the interleaved F, G at count n: f_j = F_j / n into plane j, g_j = max(0, (G_j - F_j*f_j) / (n - 1)) / n into
// plane 7 + j.  A pixel that is not FEATURE-VALID (the caller's seed, n >= 2, fourteen finite sums) gets a NaN in plane 0.
__device__ inline void feature_planes_pixel(const double *__restrict__ F, const double *__restrict__ G, size_t i, uint32_t n, bool seed, size_t N,
                                            double *__restrict__ planes) {
	const double nd = (double)n;
	bool valid = seed && n >= 2u;
	double f0 = 0.0;
#pragma unroll
	for (int j = 0; j < kDenoiseFeat; j++) { // plane 0 waits for the validity; every other plane is written as it is made (all fourteen held for one group of stores: 69 VGPRs in the region prologue)
		const double s = F[i * kDenoiseFeat + j], q = G[i * kDenoiseFeat + j];
		valid = valid && denoise_finite(s) && denoise_finite(q);
		double f, g;
		denoise_moments(s, q, nd, f, g);
		if (j == 0) f0 = f;
		else planes[(size_t)j * N + i] = f;
		planes[(size_t)(kDenoiseFeat + j) * N + i] = g;
	}
	planes[i] = valid ? f0 : __builtin_nan("");
}

// rmd_denoise_dual's combination of a dual-valid pixel's f_A = a and f_B = b: out = (n_A*f_A + n_B*f_B) / (n_A + n_B) — the two products, their sum, one
// division —, err = (h_0^2 + h_1^2 + h_2^2) / 3 with h_c = (f_Ac - f_Bc) / 2, summed in channel order.  err may be null.
__device__ inline void dual_combine(const double a[3], const double b[3], double na, double nb, size_t pix, double *__restrict__ out, double *__restrict__ err) {
	const double nsum = na + nb;
	double e = 0.0;
#pragma unroll
	for (int c = 0; c < 3; c++) {
		out[pix * 3 + c] = (na * a[c] + nb * b[c]) / nsum;
		const double h = (a[c] - b[c]) / 2.0;
		e = c == 0 ? h * h : e + h * h;
	}
	if (err) err[pix] = e / 3.0;
}
// ... and of any other pixel: the merged mean as IEEE gives it, err = NaN
__device__ inline void dual_merged(const double *__restrict__ SA, const double *__restrict__ SB, double na, double nb, size_t pix, double *__restrict__ out,
                                   double *__restrict__ err) {
	const double nsum = na + nb;
#pragma unroll
	for (int c = 0; c < 3; c++) out[pix * 3 + c] = (SA[pix * 3 + c] + SB[pix * 3 + c]) / nsum;
	if (err) err[pix] = __builtin_nan("");
}

// the frame index of pixel i (row-major within the rect) of rect r
__device__ inline size_t rect_pixel(const rmd_tile_rect &r, uint64_t i, uint32_t W) {
	const uint32_t x = (uint32_t)(i % r.width), y = (uint32_t)(i / r.width);
	return (size_t)(r.left + x) + (size_t)(r.top + y) * W;
}

} // namespace rmd
