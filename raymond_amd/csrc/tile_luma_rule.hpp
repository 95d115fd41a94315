// The rule of rmd_tile_luma_error (include/raymond_hip.h states the definition): the lines the kernel (tile_luma.hip), the C++ mirror (raymond_amd/host) and
// tests/tile_luma_rule_main.cpp all read.  Needs only <stdint.h> and despike_rule.hpp, whose validity, Y and V a pixel takes; under hipcc the functions are
// __host__ __device__.  Built without contraction (-ffp-contract=off) wherever it is built: every product is rounded, every addition is as bracketed.
#pragma once
#include <stdint.h>

#include "despike_rule.hpp"

namespace rmd {

constexpr uint32_t kTileLumaLanes = 256u, kTileLumaWave = 64u; // one workgroup of four waves per rect

// rmd_tile_luma's fields in its order (api_denoise.cpp asserts the two layouts agree): what the kernel writes and the host function returns
struct TileLuma {
	double tile_rms, pixel_rms, mean_luma, mean_variance, mean_rel_variance;
	uint32_t valid, invalid;
};

// What a lane carries, and what the combine adds: the sums of Y, V and R over valid pixels and the two counts
struct TileLumaSums {
	double sy = 0.0, sv = 0.0, sr = 0.0;
	uint32_t valid = 0u, invalid = 0u;
};

// The per-pixel step: d = max(|Y|, floor) with a NaN-proof compare, R = (V / d) / d — two divisions, no square root.  Y of a valid pixel is finite and V is
// in [0, +inf], so with floor > 0 no input makes R NaN
RMD_LUMA_HD inline void tile_luma_pixel(double Y, double V, double floor, double &d, double &R) {
	d = __builtin_fabs(Y);
	if (!(d > floor)) d = floor;
	const double vd = V / d;
	R = vd / d;
}

// One pixel into a lane's sums, in the order the lane meets its pixels
RMD_LUMA_HD inline void tile_luma_add(TileLumaSums &a, const double s[3], const double q[3], uint32_t n, double floor) {
	double Y, V, d, R;
	if (!despike_pixel(s, q, n, Y, V)) {
		a.invalid++;
		return;
	}
	tile_luma_pixel(Y, V, floor, d, R);
	a.sy = a.sy + Y, a.sv = a.sv + V, a.sr = a.sr + R;
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

// Host only.  One rect as the kernel walks it: 256 emulated lanes, lane t taking the rect's row-major pixels t, t + 256, ..., then the kernel's combine —
// within each wave of 64 the exchange with the lane 32, 16, 8, 4, 2, 1 apart, then the four waves' sums as (w0 + w1) + (w2 + w3).  S, Q: the frame's sums
// and sums of squares, 3 doubles a pixel, rows `frame_width` pixels apart; the rect lies inside the frame
inline TileLuma tile_luma_rect_host(const double *S, const double *Q, uint32_t frame_width, uint32_t left, uint32_t top, uint32_t width, uint32_t height, uint32_t n,
                                    double floor) {
	TileLumaSums lane[kTileLumaLanes];
	const uint64_t n_px = (uint64_t)width * height;
	for (uint32_t t = 0; t < kTileLumaLanes; t++)
		for (uint64_t i = t; i < n_px; i += kTileLumaLanes) {
			const uint64_t pix = (uint64_t)(left + (uint32_t)(i % width)) + (uint64_t)(top + (uint32_t)(i / width)) * frame_width;
			tile_luma_add(lane[t], S + pix * 3u, Q + pix * 3u, n, floor);
		}
	for (uint32_t off = kTileLumaWave / 2u; off > 0u; off >>= 1) {
		TileLumaSums next[kTileLumaLanes];
		for (uint32_t t = 0; t < kTileLumaLanes; t++) {
			const TileLumaSums &a = lane[t], &b = lane[t ^ off]; // (t ^ off stays inside t's wave: off < 64)
			next[t].sy = a.sy + b.sy, next[t].sv = a.sv + b.sv, next[t].sr = a.sr + b.sr;
			next[t].valid = a.valid + b.valid, next[t].invalid = a.invalid + b.invalid;
		}
		for (uint32_t t = 0; t < kTileLumaLanes; t++) lane[t] = next[t];
	}
	const TileLumaSums &w0 = lane[0], &w1 = lane[kTileLumaWave], &w2 = lane[2u * kTileLumaWave], &w3 = lane[3u * kTileLumaWave];
	return tile_luma_final((w0.sy + w1.sy) + (w2.sy + w3.sy), (w0.sv + w1.sv) + (w2.sv + w3.sv), (w0.sr + w1.sr) + (w2.sr + w3.sr),
	                       (w0.valid + w1.valid) + (w2.valid + w3.valid), (w0.invalid + w1.invalid) + (w2.invalid + w3.invalid), n_px, floor);
}

} // namespace rmd
