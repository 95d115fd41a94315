// The rule of rmd_despike (include/raymond_hip.h states the definition): the lines the kernel (despike.hip), the C++ mirror (raymond_amd/host) and
// tests/despike_rule_main.cpp all read.  Needs only <stdint.h> and luma_bins.hpp; under hipcc the functions are __host__ __device__.  Built without
// contraction (-ffp-contract=off) wherever it is built: every product is rounded, every addition is as bracketed.
#pragma once
#include <stdint.h>

#include "luma_bins.hpp"

namespace rmd {

constexpr uint32_t kDespikeMaxRadius = 3u; // a window of at most 7 x 7: 48 others

// The sums of a valid pixel are finite (and its count is >= 2)
RMD_LUMA_HD inline bool despike_finite(double x) {
	const uint64_t mag = luma_bits(x) & 0x7FFFFFFFFFFFFFFFull;
	return mag < 0x7FF0000000000000ull;
}
RMD_LUMA_HD inline bool despike_valid(const double s[3], const double q[3], uint32_t n) {
	return n >= 2u && despike_finite(s[0]) && despike_finite(s[1]) && despike_finite(s[2]) && despike_finite(q[0]) && despike_finite(q[1]) && despike_finite(q[2]);
}

// One channel's mean u = s / n and variance of the mean v = max(0, (q - s*u) / (n - 1)) / n; nd = (double)n
RMD_LUMA_HD inline void despike_moments(double s, double q, double nd, double &u, double &v) {
	u = s / nd;
	const double su = s * u;
	double t = (q - su) / (nd - 1.0);
	if (!(t > 0.0)) t = 0.0;
	v = t / nd;
}

// Y: the luminance of the means (luma_bins.hpp: luma_of)
RMD_LUMA_HD inline double despike_luma(double u0, double u1, double u2) { return luma_of(u0, u1, u2); }

// V: the variance of Y, each channel's variance under the square of its weight (the binary64 product of the weight with itself)
RMD_LUMA_HD inline double despike_luma_variance(double v0, double v1, double v2) {
	const double a0 = 0.2126 * 0.2126, a1 = 0.7152 * 0.7152, a2 = 0.0722 * 0.0722;
	const double p0 = a0 * v0, p1 = a1 * v1, p2 = a2 * v2;
	return (p0 + p1) + p2;
}

// Y and V of a pixel from its six sums and its count; false (and nothing written) for a pixel that is not valid
RMD_LUMA_HD inline bool despike_pixel(const double s[3], const double q[3], uint32_t n, double &Y, double &V) {
	if (!despike_valid(s, q, n)) return false;
	const double nd = (double)n;
	double u[3], v[3];
	for (int c = 0; c < 3; c++) despike_moments(s[c], q[c], nd, u[c], v[c]);
	Y = despike_luma(u[0], u[1], u[2]);
	V = despike_luma_variance(v[0], v[1], v[2]);
	return true;
}

// The raster index of the offset (dx, dy) in a window of `radius`: dy ascending, then dx ascending
RMD_LUMA_HD inline uint32_t despike_raster(int dx, int dy, uint32_t radius) {
	const int r = (int)radius;
	return (uint32_t)((dy + r) * (2 * r + 1) + (dx + r));
}

// The order of the others: a (luminance ya, raster index ia) stands before b if it is brighter, or as bright and earlier in raster order.  Y of a valid
// pixel is never NaN, so this is a strict total order over a window's others
RMD_LUMA_HD inline bool despike_before(double ya, uint32_t ia, double yb, uint32_t ib) { return ya > yb || (ya == yb && ia < ib); }

// The decision: p (luminance yp) against its donor (luminance yd, variance vd).  No square root; a NaN anywhere fails a comparison: no spike
RMD_LUMA_HD inline bool despike_is_spike(double yp, double yd, double vd, double k, double ratio, double floor) {
	const double rq = ratio * yd;
	const double e = (yp - rq) - floor;
	const double k2 = k * k;
	const double ee = e * e, bound = k2 * vd;
	return e > 0.0 && ee > bound;
}

// What more than `rank` others at or above yp settle without the selection: the donor is then at or above yp, and with yp >= 0, ratio >= 1 and
// floor >= 0 the rounded ratio * yd is at or above yp as well, so e <= 0 (or NaN).  For yp < 0 that does not follow — ratio * yd may lie below yd —
// and the selection is made
RMD_LUMA_HD inline bool despike_settled(uint32_t at_or_above, uint32_t rank, double yp) { return at_or_above > rank && yp >= 0.0; }

// The scaled copy: the donor's per-sample moment at p's own count
RMD_LUMA_HD inline double despike_scaled(double donor_sum, uint32_t n_donor, uint32_t n_p) {
	const double per_sample = donor_sum / (double)n_donor;
	return per_sample * (double)n_p;
}

// A window is its (2 * radius + 1)^2 luminances in rows `stride` doubles apart, win[0] the offset (-radius, -radius); the centre is p itself and is
// skipped, and a NaN marks a position that is no other: outside the frame, or a pixel that is not valid.
//
// The others at or above yp, which despike_settled takes
RMD_LUMA_HD inline uint32_t despike_at_or_above(const double *win, uint32_t stride, uint32_t radius, double yp) {
	const uint32_t side = 2u * radius + 1u;
	uint32_t n = 0;
	for (uint32_t row = 0; row < side; row++)
		for (uint32_t col = 0; col < side; col++)
			if (!(row == radius && col == radius) && win[row * stride + col] >= yp) n++;
	return n;
}
// The donor: the raster index of the other at 0-based index `rank` of the order, or -1 when there are fewer than rank + 1 others.  rank + 1 passes over
// the window, each taking the first other that stands after the one taken before
RMD_LUMA_HD inline int despike_donor(const double *win, uint32_t stride, uint32_t radius, uint32_t rank) {
	const uint32_t side = 2u * radius + 1u, centre = radius * side + radius;
	double prev_y = 0.0;
	uint32_t prev_i = 0;
	bool has_prev = false;
	for (uint32_t t = 0; t <= rank; t++) {
		double best_y = 0.0;
		uint32_t best_i = 0;
		bool has_best = false;
		for (uint32_t row = 0, i = 0; row < side; row++)
			for (uint32_t col = 0; col < side; col++, i++) {
				const double yq = win[row * stride + col];
				if (i == centre || !(yq == yq)) continue;
				if (has_prev && !despike_before(prev_y, prev_i, yq, i)) continue;
				if (!has_best || despike_before(yq, i, best_y, best_i)) best_y = yq, best_i = i, has_best = true;
			}
		if (!has_best) return -1;
		prev_y = best_y, prev_i = best_i, has_prev = true;
	}
	return (int)prev_i;
}

} // namespace rmd
