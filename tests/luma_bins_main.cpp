// Drives raymond_amd/csrc/luma_bins.hpp — the binning of rmd_luminance_histogram_tiles, the lines its kernel is built from — on the CPU
// (tests/test_luminance_histogram_host.py builds this with -fsanitize=address,undefined and runs it directly).
//
//   luma_bins <seed> <random patterns>
//
// luma_counter makes a counter from a double's 64 bits alone.  Here every result is held against a second reading that never looks at the bits: isnan /
// isinf, comparisons with 0, and frexp — y = m * 2^e with 0.5 <= m < 1, so the unbiased exponent is E = e - 1 and the top two mantissa bits are
// M = floor((2 m - 1) * 4), both exact (frexp normalises denormals, and a scaling by a power of two rounds nothing).  Values:
//   * every bin edge ldexp(1 + m / 4, e) for e in -34 .. 33 and m in 0 .. 3 — two octaves past either end of the bins —, the double just below it and
//     the double just above it; an edge must open its own bin, the double below it must close the bin before;
//   * +-0, the smallest and the largest denormal, DBL_MIN, DBL_MAX, +-inf, quiet and signalling NaN patterns of either sign, negatives;
//   * <random patterns> random 64-bit patterns (every class of double: an exponent field drawn uniformly).
// It also checks luma_of against the three rounded products and two additions written out, volatile between them so that nothing is fused.
#include <cfloat>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "luma_bins.hpp"

static double from_bits(uint64_t bits) {
	double y;
	std::memcpy(&y, &bits, sizeof(y));
	return y;
}

// The counter of y, read without its bits
static uint32_t by_frexp(double y) {
	if (std::isnan(y) || std::isinf(y)) return rmd::kLumaNotFinite;
	if (y == 0.0) return rmd::kLumaZero;
	if (y < 0.0) return rmd::kLumaNegative;
	int e = 0;
	const double m = std::frexp(y, &e);
	const int E = e - 1;
	if (E < -32) return rmd::kLumaBelow;
	if (E >= 32) return rmd::kLumaAbove;
	const int M = (int)std::floor((2.0 * m - 1.0) * 4.0);
	return (uint32_t)((E + 32) * 4 + M);
}

static uint64_t checked = 0;
static bool same(double y, const char *what) {
	const uint32_t got = rmd::luma_counter(rmd::luma_bits(y)), want = by_frexp(y);
	checked++;
	if (got == want) return true;
	std::fprintf(stderr, "%s: %a (bits %016" PRIx64 ") is counted in %u, frexp reads %u\n", what, y, rmd::luma_bits(y), got, want);
	return false;
}

int main(int argc, char **argv) {
	const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1, n_random = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1000000;
	static_assert(rmd::kLumaBins == 256 && rmd::kLumaCounters == 261, "64 octaves of four bins and five side counters");
	bool ok = true;
	for (int e = -34; e <= 33; e++)
		for (int m = 0; m < 4; m++) {
			const double edge = std::ldexp(1.0 + m / 4.0, e), under = std::nextafter(edge, 0.0), over = std::nextafter(edge, HUGE_VAL);
			ok = same(edge, "edge") && same(under, "below an edge") && same(over, "above an edge") && ok;
			const uint32_t at = rmd::luma_counter(rmd::luma_bits(edge)), before = rmd::luma_counter(rmd::luma_bits(under));
			if (e >= -32 && e < 32) {
				const uint32_t bin = (uint32_t)((e + 32) * 4 + m);
				const uint32_t prev = bin == 0 ? rmd::kLumaBelow : bin - 1;
				if (at != bin || before != prev || rmd::luma_counter(rmd::luma_bits(over)) != bin) {
					std::fprintf(stderr, "edge %a: counted in %u (bin %u), the double below it in %u (want %u)\n", edge, at, bin, before, prev);
					ok = false;
				}
			} else if (at != (e < -32 ? rmd::kLumaBelow : rmd::kLumaAbove)) {
				std::fprintf(stderr, "edge %a outside the bins is counted in %u\n", edge, at);
				ok = false;
			}
		}
	if (rmd::luma_counter(rmd::luma_bits(std::nextafter(0x1p32, 0.0))) != 255u || rmd::luma_counter(rmd::luma_bits(0x1p32)) != rmd::kLumaAbove) {
		std::fprintf(stderr, "the last bin does not end at 2^32\n");
		ok = false;
	}
	const uint64_t specials[] = {0x0000000000000000ull, 0x8000000000000000ull,                         // +-0
	                             0x0000000000000001ull, 0x000FFFFFFFFFFFFFull,                         // the smallest and the largest denormal
	                             0x8000000000000001ull, 0x800FFFFFFFFFFFFFull,                         // ... negative
	                             0x7FF0000000000000ull, 0xFFF0000000000000ull,                         // +-inf
	                             0x7FF8000000000000ull, 0xFFF8000000000000ull, 0x7FF8000000000001ull,  // quiet NaNs
	                             0x7FF0000000000001ull, 0xFFF0000000000001ull, 0x7FF7FFFFFFFFFFFFull,  // signalling NaNs
	                             0x7FFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFFull};
	for (uint64_t bits : specials) ok = same(from_bits(bits), "special") && ok;
	const double values[] = {DBL_MIN, DBL_MAX, -DBL_MIN, -DBL_MAX, -1.0, -1.75, -0x1p-40, -0x1p40, 1.0, 1.75, 0.18, 1e-300, 1e300};
	for (double y : values) ok = same(y, "value") && ok;
	const struct { uint64_t bits; uint32_t counter; } pins[] = {
	    {0x0000000000000000ull, rmd::kLumaZero},      {0x8000000000000000ull, rmd::kLumaZero},      {0x0000000000000001ull, rmd::kLumaBelow},
	    {0x000FFFFFFFFFFFFFull, rmd::kLumaBelow},     {0x0010000000000000ull, rmd::kLumaBelow},     {0x7FEFFFFFFFFFFFFFull, rmd::kLumaAbove},
	    {0x7FF0000000000000ull, rmd::kLumaNotFinite}, {0xFFF0000000000000ull, rmd::kLumaNotFinite}, {0x7FF0000000000001ull, rmd::kLumaNotFinite},
	    {0xFFF8000000000000ull, rmd::kLumaNotFinite}, {0x8000000000000001ull, rmd::kLumaNegative},  {0xBFF0000000000000ull, rmd::kLumaNegative},
	    {0x3FF0000000000000ull, 128u},                {0x3FFC000000000000ull, 131u}};
	for (const auto &p : pins)
		if (rmd::luma_counter(p.bits) != p.counter) {
			std::fprintf(stderr, "bits %016" PRIx64 " are counted in %u, not %u\n", p.bits, rmd::luma_counter(p.bits), p.counter);
			ok = false;
		}
	std::mt19937_64 rng(seed);
	uint64_t seen[rmd::kLumaCounters] = {};
	for (uint64_t i = 0; i < n_random && ok; i++) {
		const uint64_t bits = rng();
		ok = same(from_bits(bits), "random pattern") && ok;
		seen[rmd::luma_counter(bits)]++;
	}
	uint32_t hit = 0;
	for (uint32_t i = 0; i < rmd::kLumaCounters; i++) hit += seen[i] != 0;
	// the luminance: three rounded products, the first two added, then the third
	for (int i = 0; i < 100000 && ok; i++) {
		const double r = from_bits(rng()), g = from_bits(rng()), b = (i & 1) ? from_bits(rng()) : std::ldexp((double)(rng() >> 11), -40);
		volatile double pr = 0.2126 * r, pg = 0.7152 * g, pb = 0.0722 * b;
		volatile double s = pr + pg;
		const double want = s + pb, got = rmd::luma_of(r, g, b);
		if (rmd::luma_bits(want) != rmd::luma_bits(got) && !(std::isnan(want) && std::isnan(got))) {
			std::fprintf(stderr, "luma_of(%a, %a, %a) = %a, the operations written out give %a\n", r, g, b, got, want);
			ok = false;
		}
	}
	if (!ok) return 1;
	std::printf("luma bins ok: %" PRIu64 " values, %u of %u counters hit by the random patterns\n", checked, hit, rmd::kLumaCounters);
	return 0;
}
