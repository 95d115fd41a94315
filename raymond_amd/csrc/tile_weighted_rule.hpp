// The rule of rmd_tile_weighted_error (include/raymond_hip.h states the definition): the lines the kernel (tile_weighted.hip), the C++ mirror
// (raymond_amd/host) and tests/tile_weighted_rule_main.cpp all read.  Needs only <stdint.h>, luma_bins.hpp — whose counter of a luminance's bits picks the
// pixel's weight — and despike_rule.hpp, whose validity, Y and V a pixel takes; under hipcc the functions are __host__ __device__.  Built without
// contraction (-ffp-contract=off) wherever it is built: every product is rounded, every addition is as bracketed.  No library function but the final
// square root: a pixel is a table lookup, one product and three additions.
#pragma once
#include <stdint.h>

#include "luma_bins.hpp"
#include "despike_rule.hpp"

namespace rmd {

constexpr uint32_t kTileWeightedLanes = 256u, kTileWeightedWave = 64u; // one workgroup of four waves per rect
constexpr uint32_t kLumaWeights = 260u;                                // RMD_LUMA_WEIGHTS: luma_bins.hpp's counters without kLumaNotFinite
static_assert(kLumaWeights == kLumaNotFinite && kLumaWeights == kLumaCounters - 1u, "a weight per counter of luma_bins.hpp, not_finite left out");

// rmd_tile_weighted's fields in its order (api_denoise.cpp asserts the two layouts agree): what the kernel writes and the host function returns
struct TileWeighted {
	double rms, mean_weighted_variance, mean_luma, mean_variance;
	uint32_t valid, invalid;
};

// What a lane carries, and what the combine adds: the sums of Y, V and E over valid pixels and the two counts
struct TileWeightedSums {
	double sy = 0.0, sv = 0.0, se = 0.0;
	uint32_t valid = 0u, invalid = 0u;
};

// The per-pixel step: the weighted variance E of a pixel with luminance counter k < kLumaWeights.  One rounded product; a zero weight gives +0.0 whatever
// V is (V may be +inf, and a saturated bin's weight is 0).  weights: kLumaWeights entries, each finite and >= 0, so E is never NaN
RMD_LUMA_HD inline double tile_weighted_pixel(double V, uint32_t k, const double *weights) {
	const double w = weights[k];
	return (w == 0.0) ? 0.0 : w * V;
}

// One pixel into a lane's sums, in the order the lane meets its pixels.  A valid pixel whose counter is kLumaNotFinite (its luminance overflowed: the sums
// are finite, their weighted sum is not) counts as invalid
RMD_LUMA_HD inline void tile_weighted_add(TileWeightedSums &a, const double s[3], const double q[3], uint32_t n, const double *weights) {
	double Y, V;
	if (!despike_pixel(s, q, n, Y, V)) {
		a.invalid++;
		return;
	}
	const uint32_t k = luma_counter(luma_bits(Y));
	if (k >= kLumaWeights) {
		a.invalid++;
		return;
	}
	const double E = tile_weighted_pixel(V, k, weights);
	a.sy = a.sy + Y, a.sv = a.sv + V, a.se = a.se + E;
	a.valid++;
}

// The final step: the rect's sums and counts -> the result's fields.  n_px: the rect's pixels (valid + invalid)
RMD_LUMA_HD inline TileWeighted tile_weighted_final(double SY, double SV, double SE, uint32_t valid, uint32_t invalid, uint64_t n_px) {
	TileWeighted o;
	o.valid = valid, o.invalid = invalid;
	if (n_px == 0u) { // a rect without pixels: all zeros
		o.rms = o.mean_weighted_variance = o.mean_luma = o.mean_variance = 0.0;
		return o;
	}
	const double m = (double)valid;
	o.mean_luma = valid ? SY / m : 0.0;
	o.mean_variance = valid ? SV / m : 0.0;
	o.mean_weighted_variance = valid ? SE / m : 0.0;
	o.rms = __builtin_sqrt(o.mean_weighted_variance);
	if (invalid != 0u) o.rms = __builtin_inf(); // a tile with a bad pixel never finishes on this rule
	if (!(o.rms == o.rms)) o.rms = __builtin_inf();
	return o;
}

// Host only.  One rect as the kernel walks it: 256 emulated lanes, lane t taking the rect's row-major pixels t, t + 256, ..., then the kernel's combine —
// within each wave of 64 the exchange with the lane 32, 16, 8, 4, 2, 1 apart, then the four waves' sums as (w0 + w1) + (w2 + w3).  S, Q: the frame's sums
// and sums of squares, 3 doubles a pixel, rows `frame_width` pixels apart; the rect lies inside the frame; weights: kLumaWeights entries
inline TileWeighted tile_weighted_rect_host(const double *S, const double *Q, uint32_t frame_width, uint32_t left, uint32_t top, uint32_t width, uint32_t height,
                                            uint32_t n, const double *weights) {
	TileWeightedSums lane[kTileWeightedLanes];
	const uint64_t n_px = (uint64_t)width * height;
	for (uint32_t t = 0; t < kTileWeightedLanes; t++)
		for (uint64_t i = t; i < n_px; i += kTileWeightedLanes) {
			const uint64_t pix = (uint64_t)(left + (uint32_t)(i % width)) + (uint64_t)(top + (uint32_t)(i / width)) * frame_width;
			tile_weighted_add(lane[t], S + pix * 3u, Q + pix * 3u, n, weights);
		}
	for (uint32_t off = kTileWeightedWave / 2u; off > 0u; off >>= 1) {
		TileWeightedSums next[kTileWeightedLanes];
		for (uint32_t t = 0; t < kTileWeightedLanes; t++) {
			const TileWeightedSums &a = lane[t], &b = lane[t ^ off]; // (t ^ off stays inside t's wave: off < 64)
			next[t].sy = a.sy + b.sy, next[t].sv = a.sv + b.sv, next[t].se = a.se + b.se;
			next[t].valid = a.valid + b.valid, next[t].invalid = a.invalid + b.invalid;
		}
		for (uint32_t t = 0; t < kTileWeightedLanes; t++) lane[t] = next[t];
	}
	const TileWeightedSums &w0 = lane[0], &w1 = lane[kTileWeightedWave], &w2 = lane[2u * kTileWeightedWave], &w3 = lane[3u * kTileWeightedWave];
	return tile_weighted_final((w0.sy + w1.sy) + (w2.sy + w3.sy), (w0.sv + w1.sv) + (w2.sv + w3.sv), (w0.se + w1.se) + (w2.se + w3.se),
	                           (w0.valid + w1.valid) + (w2.valid + w3.valid), (w0.invalid + w1.invalid) + (w2.invalid + w3.invalid), n_px);
}

} // namespace rmd
