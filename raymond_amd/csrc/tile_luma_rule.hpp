// The rule of rmd_tile_luma_error (include/raymond_hip.h states the definition): the lines the kernel (tile_luma.hip), the C++ mirror (raymond_amd/host) and
// tests/tile_luma_rule_main.cpp all read.  Needs only <stdint.h>, despike_rule.hpp, whose validity, Y and V a pixel takes, and tile_reduce.hpp, whose order
// the sums are added in; under hipcc the functions are __host__ __device__.  Built without contraction (-ffp-contract=off) wherever it is built: every
// product is rounded, every addition is as bracketed.
#pragma once
#include <stdint.h>

#include "despike_rule.hpp"
#include "tile_reduce.hpp"

namespace rmd {

// rmd_tile_luma's fields in its order (api_denoise.cpp asserts the two layouts agree): what the kernel writes and the host function returns
struct TileLuma {
	double tile_rms, pixel_rms, mean_luma, mean_variance, mean_rel_variance;
	uint32_t valid, invalid;
};

// The per-pixel step: d = max(|Y|, floor) with a NaN-proof compare, R = (V / d) / d — two divisions, no square root.  Y of a valid pixel is finite and V is
// in [0, +inf], so with floor > 0 no input makes R NaN
RMD_LUMA_HD inline void tile_luma_pixel(double Y, double V, double floor, double &d, double &R) {
	d = __builtin_fabs(Y);
	if (!(d > floor)) d = floor;
	const double vd = V / d;
	R = vd / d;
}

// One pixel into a lane's sums, in the order the lane meets its pixels; the sums' own term (se) is R
RMD_LUMA_HD inline void tile_luma_add(TileSums &a, const double s[3], const double q[3], uint32_t n, double floor) {
	double Y, V, d, R;
	if (!despike_pixel(s, q, n, Y, V)) {
		a.invalid++;
		return;
	}
	tile_luma_pixel(Y, V, floor, d, R);
	a.sy = a.sy + Y, a.sv = a.sv + V, a.se = a.se + R;
	a.valid++;
}

// The final step: the rect's sums and counts -> the result's fields.  n_px: the rect's pixels (valid + invalid)
RMD_LUMA_HD inline TileLuma tile_luma_final(double SY, double SV, double SR, uint32_t valid, uint32_t invalid, uint64_t n_px, double floor) {
	TileLuma o;
	o.valid = valid, o.invalid = invalid;
	if (n_px == 0u) { // a rect without pixels: all zeros
		o.tile_rms = o.pixel_rms = o.mean_luma = o.mean_variance = o.mean_rel_variance = 0.0;
		return o;
	}
	const double m = (double)valid;
	o.mean_luma = valid ? SY / m : 0.0;
	o.mean_variance = valid ? SV / m : 0.0;
	o.mean_rel_variance = valid ? SR / m : 0.0;
	double D = __builtin_fabs(o.mean_luma);
	if (!(D > floor)) D = floor;
	o.tile_rms = __builtin_sqrt(o.mean_variance) / D;
	o.pixel_rms = __builtin_sqrt(o.mean_rel_variance);
	if (invalid != 0u) o.tile_rms = o.pixel_rms = __builtin_inf(); // a tile with a bad pixel never finishes on this rule
	if (!(o.tile_rms == o.tile_rms)) o.tile_rms = __builtin_inf(); // inf / inf when the sums overflow
	if (!(o.pixel_rms == o.pixel_rms)) o.pixel_rms = __builtin_inf();
	return o;
}

// Host only.  One rect as the kernel walks it (tile_reduce.hpp: tile_rect_sums_host).  S, Q: the frame's sums and sums of squares, 3 doubles a pixel, rows
// `frame_width` pixels apart; the rect lies inside the frame
inline TileLuma tile_luma_rect_host(const double *S, const double *Q, uint32_t frame_width, uint32_t left, uint32_t top, uint32_t width, uint32_t height, uint32_t n,
                                    double floor) {
	const TileSums a = tile_rect_sums_host(frame_width, left, top, width, height, [&](TileSums &lane, uint64_t pix) { tile_luma_add(lane, S + pix * 3u, Q + pix * 3u, n, floor); });
	return tile_luma_final(a.sy, a.sv, a.se, a.valid, a.invalid, (uint64_t)width * height, floor);
}

} // namespace rmd
