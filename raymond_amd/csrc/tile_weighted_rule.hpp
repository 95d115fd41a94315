// The rule of rmd_tile_weighted_error (include/raymond_hip.h states the definition): the lines the kernel (tile_weighted.hip), the C++ mirror
// (raymond_amd/host) and tests/tile_weighted_rule_main.cpp all read.  Needs only <stdint.h>, luma_bins.hpp — whose counter of a luminance's bits picks the
// pixel's weight —, despike_rule.hpp, whose validity, Y and V a pixel takes, and tile_reduce.hpp, whose order the sums are added in; under hipcc the
// functions are __host__ __device__.  Built without contraction (-ffp-contract=off) wherever it is built: every product is rounded, every addition is as
// bracketed.  No library function but the final square root: a pixel is a table lookup, one product and three additions.
#pragma once
#include <stdint.h>

#include "luma_bins.hpp"
#include "despike_rule.hpp"
#include "tile_reduce.hpp"

namespace rmd {

constexpr uint32_t kLumaWeights = 260u; // RMD_LUMA_WEIGHTS: luma_bins.hpp's counters without kLumaNotFinite
static_assert(kLumaWeights == kLumaNotFinite && kLumaWeights == kLumaCounters - 1u, "a weight per counter of luma_bins.hpp, not_finite left out");

// rmd_tile_weighted's fields in its order (api_denoise.cpp asserts the two layouts agree): what the kernel writes and the host function returns
struct TileWeighted {
	double rms, mean_weighted_variance, mean_luma, mean_variance;
	uint32_t valid, invalid;
};

using TileWeightedSums = TileSums; // (the name the rule's main knows the sums by; their own term, se, is E)

// The per-pixel step: the weighted variance E of a pixel with luminance counter k < kLumaWeights.  One rounded product; a zero weight gives +0.0 whatever
// V is (V may be +inf, and a saturated bin's weight is 0).  weights: kLumaWeights entries, each finite and >= 0, so E is never NaN
RMD_LUMA_HD inline double tile_weighted_pixel(double V, uint32_t k, const double *weights) {
	const double w = weights[k];
	return (w == 0.0) ? 0.0 : w * V;
}

// One pixel into a lane's sums, in the order the lane meets its pixels.  A valid pixel whose counter is kLumaNotFinite (its luminance overflowed: the sums
// are finite, their weighted sum is not) counts as invalid
RMD_LUMA_HD inline void tile_weighted_add(TileSums &a, const double s[3], const double q[3], uint32_t n, const double *weights) {
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

// Host only.  One rect as the kernel walks it (tile_reduce.hpp: tile_rect_sums_host).  S, Q: the frame's sums and sums of squares, 3 doubles a pixel, rows
// `frame_width` pixels apart; the rect lies inside the frame; weights: kLumaWeights entries
inline TileWeighted tile_weighted_rect_host(const double *S, const double *Q, uint32_t frame_width, uint32_t left, uint32_t top, uint32_t width, uint32_t height,
                                            uint32_t n, const double *weights) {
	const TileSums a = tile_rect_sums_host(frame_width, left, top, width, height, [&](TileSums &lane, uint64_t pix) { tile_weighted_add(lane, S + pix * 3u, Q + pix * 3u, n, weights); });
	return tile_weighted_final(a.sy, a.sv, a.se, a.valid, a.invalid, (uint64_t)width * height);
}

} // namespace rmd
