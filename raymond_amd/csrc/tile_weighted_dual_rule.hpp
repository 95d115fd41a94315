// The rule of rmd_tile_weighted_error_dual (include/raymond_hip.h states the definition): the lines the kernel (tile_weighted_dual.hip), the C++ mirror
// (raymond_amd/host) and tests/tile_weighted_dual_rule_main.cpp all read.  Needs only <stdint.h> and tile_weighted_rule.hpp, whose weighted term, final
// step and — through tile_reduce.hpp — summation order it takes unchanged; under hipcc the functions are __host__ __device__.  Built without contraction
// (-ffp-contract=off) wherever it is built.  No library function: a pixel is a luminance of three means, a table lookup, one product and three additions.
#pragma once
#include <stdint.h>

#include "tile_weighted_rule.hpp"

namespace rmd {

// One pixel of the FILTERED frame into a lane's sums, in the order the lane meets its pixels.  o: the pixel's three filtered means; e: its entry of the
// dual filter's error image, the variance that is weighed.  Valid: e is not NaN (a pixel that is not dual-valid has e = NaN) and the three means are
// finite; e = +inf is valid, a negative e is added as it is.  A valid pixel whose luminance overflowed (counter kLumaNotFinite) counts as invalid.
// tile_weighted_pixel's zero-weight guard is reachable here: e may be +inf under a weight of 0
RMD_LUMA_HD inline void tile_weighted_dual_add(TileSums &a, const double o[3], double e, const double *weights) {
	if (!(e == e) || !despike_finite(o[0]) || !despike_finite(o[1]) || !despike_finite(o[2])) {
		a.invalid++;
		return;
	}
	const double Y = despike_luma(o[0], o[1], o[2]);
	const uint32_t k = luma_counter(luma_bits(Y));
	if (k >= kLumaWeights) {
		a.invalid++;
		return;
	}
	const double E = tile_weighted_pixel(e, k, weights);
	a.sy = a.sy + Y, a.sv = a.sv + e, a.se = a.se + E;
	a.valid++;
}

// Host only.  One rect as the kernel walks it (tile_reduce.hpp: tile_rect_sums_host).  out: the filtered frame, 3 doubles a pixel; err: the error image,
// one double a pixel; rows `frame_width` pixels apart; the rect lies inside the frame; weights: kLumaWeights entries
inline TileWeighted tile_weighted_dual_rect_host(const double *out, const double *err, uint32_t frame_width, uint32_t left, uint32_t top, uint32_t width,
                                                 uint32_t height, const double *weights) {
	const TileSums a = tile_rect_sums_host(frame_width, left, top, width, height, [&](TileSums &lane, uint64_t pix) { tile_weighted_dual_add(lane, out + pix * 3u, err[pix], weights); });
	return tile_weighted_final(a.sy, a.sv, a.se, a.valid, a.invalid, (uint64_t)width * height);
}

} // namespace rmd
