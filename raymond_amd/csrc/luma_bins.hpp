// The luminance and the binning of rmd_luminance_histogram_tiles (include/raymond_hip.h states the definition): the lines the kernel
// (luma_histogram.hip), the C++ mirror's host histogram (raymond_amd/host: raymond::luminance_histogram) and tests/luma_bins_main.cpp all read.  Needs
// only <stdint.h>; under hipcc the functions are __host__ __device__.
//
// A counter index is made from the 64 bits of Y alone — no log, no comparison of doubles — so every counter is an exact integer that any host can restate:
//   E = the unbiased exponent, M = the top two mantissa bits; -32 <= E < 32: counter (E + 32) * 4 + M, a bin [2^E (1 + M / 4), 2^E (1 + (M + 1) / 4));
//   positive finite Y below 2^-32 (denormals included): kLumaBelow; at or over 2^32: kLumaAbove; +-0: kLumaZero; Y < 0: kLumaNegative;
//   NaN of either sign and +-inf: kLumaNotFinite.
// The counters' order is rmd_luma_histogram's field order, `pixels` left out.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RMD_LUMA_HD __host__ __device__
#else
#define RMD_LUMA_HD
#endif

namespace rmd {

constexpr uint32_t kLumaBins = 256u; // RMD_LUMA_BINS: 64 octaves, 2^-32 .. 2^32, four bins each
constexpr uint32_t kLumaBelow = 256u, kLumaAbove = 257u, kLumaZero = 258u, kLumaNegative = 259u, kLumaNotFinite = 260u;
constexpr uint32_t kLumaCounters = 261u;
constexpr int kLumaMinExponent = -32; // bin 0 starts at 2^-32

// The counter of the double whose bits are `bits`
RMD_LUMA_HD inline uint32_t luma_counter(uint64_t bits) {
	const uint64_t mag = bits & 0x7FFFFFFFFFFFFFFFull;
	if (mag >= 0x7FF0000000000000ull) return kLumaNotFinite; // +-inf and every NaN, whatever its sign and payload
	if (mag == 0) return kLumaZero;
	if (bits >> 63) return kLumaNegative;
	const uint32_t biased = (uint32_t)(mag >> 52); // 0: a denormal
	if (biased < (uint32_t)(1023 + kLumaMinExponent)) return kLumaBelow;
	if (biased >= (uint32_t)(1023 - kLumaMinExponent)) return kLumaAbove;
	return (biased - (uint32_t)(1023 + kLumaMinExponent)) * 4u + (uint32_t)((mag >> 50) & 3u);
}

RMD_LUMA_HD inline uint64_t luma_bits(double y) {
	uint64_t bits;
	__builtin_memcpy(&bits, &y, sizeof(bits));
	return bits;
}

// Rec. 709 luminance of linear RGB: three rounded products, then the two additions as bracketed.  Built without contraction (-ffp-contract=off) wherever
// it is built, so that no multiply-add is fused.
RMD_LUMA_HD inline double luma_of(double r, double g, double b) {
	const double pr = 0.2126 * r, pg = 0.7152 * g, pb = 0.0722 * b;
	return (pr + pg) + pb;
}

} // namespace rmd
