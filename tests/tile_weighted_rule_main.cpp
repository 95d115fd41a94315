// Drives raymond_amd/csrc/tile_weighted_rule.hpp — the rule of rmd_tile_weighted_error, the lines its kernel is built from — on the CPU
// (tests/test_tile_weighted_host.py builds this with -fsanitize=address,undefined and runs it directly).
//
//   tile_weighted_rule <seed> <random rects>
//
// Every random rect — width and height 0 .. 40, a count from {0, 1, 2, 3, 2^32 - 1}, sums with zeros of both signs, negatives, infinities and NaN among
// them at scales 2^-500 .. 2^500, in a frame that ends exactly where the rect ends so that a read past it is the sanitizer's, under a weight table of
// exactly 260 heap doubles that is random, all zero, all ones or the tone curve's (rmd_display_weights' formula) — goes through tile_weighted_rect_host
// and through a second plain reading below: the arithmetic of a pixel written out, the counter from comparisons of doubles instead of bits, an explicit
// array of 256 partials filled pixel by pixel, and an explicit tree.  The two must agree bit for bit.  Held as well: no field is NaN; invalid > 0 gives
// rms = +inf; valid + invalid is the rect's pixel count; a rect without pixels gives all zeros; a count below 2 makes every pixel invalid; an all-zero
// table gives rms 0; and the per-pixel step gives 0 for w = 0 under V = +inf.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "tile_weighted_rule.hpp"

static int failures = 0;
#define EXPECT(cond, ...)                         \
	do {                                          \
		if (!(cond)) {                            \
			if (failures++ < 20) {                \
				std::printf("FAILED %s: ", #cond); \
				std::printf(__VA_ARGS__);         \
				std::printf("\n");                \
			}                                     \
		}                                         \
	} while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

// The second reading.  The counter of a luminance from comparisons and frexp, not from its bits; 260: not finite
static uint32_t plain_counter(double y) {
	if (!std::isfinite(y)) return 260u;
	if (y == 0.0) return 258u;
	if (y < 0.0) return 259u;
	if (y < std::ldexp(1.0, -32)) return 256u;
	if (y >= std::ldexp(1.0, 32)) return 257u;
	int e;
	const double f = std::frexp(y, &e); // y = f * 2^e, f in [0.5, 1): the mantissa 1.xx is 2 f, the unbiased exponent e - 1
	const uint32_t m = 2.0 * f >= 1.75 ? 3u : 2.0 * f >= 1.5 ? 2u : 2.0 * f >= 1.25 ? 1u : 0u;
	return (uint32_t)(e - 1 + 32) * 4u + m;
}
// A pixel: validity, Y, V and E written out
static bool plain_pixel(const double *s, const double *q, uint32_t n, const std::vector<double> &weights, double &Y, double &V, double &E) {
	if (n < 2u) return false;
	for (int c = 0; c < 3; c++)
		if (!std::isfinite(s[c]) || !std::isfinite(q[c])) return false;
	const double nd = (double)n;
	double u[3], v[3];
	for (int c = 0; c < 3; c++) {
		u[c] = s[c] / nd;
		const double su = s[c] * u[c];
		const double t = (q[c] - su) / (nd - 1.0);
		v[c] = (t > 0.0 ? t : 0.0) / nd;
	}
	const double y0 = 0.2126 * u[0], y1 = 0.7152 * u[1], y2 = 0.0722 * u[2];
	Y = (y0 + y1) + y2;
	const double a0 = 0.2126 * 0.2126, a1 = 0.7152 * 0.7152, a2 = 0.0722 * 0.0722;
	const double p0 = a0 * v[0], p1 = a1 * v[1], p2 = a2 * v[2];
	V = (p0 + p1) + p2;
	const uint32_t k = plain_counter(Y);
	if (k >= 260u) return false;
	const double w = weights.at(k);
	E = w == 0.0 ? 0.0 : w * V;
	return true;
}
// 256 partials -> one: per wave of 64, the upper half onto the lower at 32, 16, 8, 4, 2, 1; then (w0 + w1) + (w2 + w3)
template <class T>
static T plain_tree(const T (&partial)[256]) {
	T wave[4];
	for (int w = 0; w < 4; w++) {
		T v[64];
		for (int l = 0; l < 64; l++) v[l] = partial[64 * w + l];
		for (int off = 32; off >= 1; off /= 2)
			for (int l = 0; l < off; l++) v[l] = v[l] + v[l + off];
		wave[w] = v[0];
	}
	return (wave[0] + wave[1]) + (wave[2] + wave[3]);
}
static rmd::TileWeighted plain_rect(const double *S, const double *Q, uint32_t frame_width, uint32_t left, uint32_t top, uint32_t width, uint32_t height, uint32_t n,
                                    const std::vector<double> &weights) {
	double py[256] = {}, pv[256] = {}, pe[256] = {};
	uint32_t valid[256] = {}, invalid[256] = {};
	uint64_t i = 0;
	for (uint32_t y = 0; y < height; y++)
		for (uint32_t x = 0; x < width; x++, i++) { // row-major within the rect: pixel i belongs to lane i % 256, which meets its pixels in ascending i
			const size_t pix = (size_t)(left + x) + (size_t)(top + y) * frame_width;
			double Y, V, E;
			if (plain_pixel(S + pix * 3, Q + pix * 3, n, weights, Y, V, E)) py[i % 256] += Y, pv[i % 256] += V, pe[i % 256] += E, valid[i % 256]++;
			else invalid[i % 256]++;
		}
	const double inf = std::numeric_limits<double>::infinity();
	rmd::TileWeighted o{};
	o.valid = plain_tree(valid), o.invalid = plain_tree(invalid);
	if (i == 0) return o;
	const double SY = plain_tree(py), SV = plain_tree(pv), SE = plain_tree(pe), m = (double)o.valid;
	o.mean_luma = o.valid ? SY / m : 0.0, o.mean_variance = o.valid ? SV / m : 0.0, o.mean_weighted_variance = o.valid ? SE / m : 0.0;
	o.rms = std::sqrt(o.mean_weighted_variance);
	if (o.invalid) o.rms = inf;
	if (std::isnan(o.rms)) o.rms = inf;
	return o;
}
// rmd_display_weights' formula: the squared slope of (1 - exp(-y e))^(1/g) per counter, capped at the luminance that displays at `floor`
static std::vector<double> display_table(double e, double g, double floor) {
	const double y_floor = -std::log1p(-std::pow(floor, g)) / e;
	auto weight = [&](double y) {
		const double t = -std::expm1(-y * e), slope = (1.0 / g) * std::pow(t, 1.0 / g - 1.0) * e * std::exp(-y * e), w = slope * slope;
		return std::isnan(w) ? 0.0 : w > std::numeric_limits<double>::max() ? std::numeric_limits<double>::max() : w;
	};
	std::vector<double> out(rmd::kLumaWeights);
	for (uint32_t i = 0; i < 256u; i++) {
		const double y = std::ldexp(1.0 + ((double)(i % 4u) + 0.5) * 0.25, (int)(i / 4u) - 32);
		out[i] = weight(y > y_floor ? y : y_floor);
	}
	out[256] = out[258] = out[259] = weight(y_floor);
	out[257] = weight(std::ldexp(1.0, 32));
	return out;
}

int main(int argc, char **argv) {
	const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
	const uint64_t n_random = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 10000;
	std::mt19937_64 rng(seed);
	const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
	const uint32_t count_set[] = {0u, 1u, 2u, 3u, 0xFFFFFFFFu};
	std::uniform_real_distribution<double> unit(0.0, 1.0);
	uint64_t rects = 0, empty = 0, with_invalid = 0, all_valid = 0, zero_rms = 0, infinite_valid = 0;

	// the counter from the bits against the counter from comparisons, on every bin's edge, the double under it, and the side counters' edges
	for (uint32_t i = 0; i <= 256u; i++) {
		const double edge = std::ldexp(1.0 + (double)(i % 4u) * 0.25, (int)(i / 4u) - 32), under = std::nextafter(edge, 0.0);
		EXPECT(rmd::luma_counter(rmd::luma_bits(edge)) == (i < 256u ? i : 257u) && plain_counter(edge) == (i < 256u ? i : 257u), "edge %u", i);
		EXPECT(rmd::luma_counter(rmd::luma_bits(under)) == (i > 0u ? i - 1u : 256u) && plain_counter(under) == (i > 0u ? i - 1u : 256u), "under edge %u", i);
	}
	EXPECT(rmd::luma_counter(rmd::luma_bits(0.0)) == 258u && rmd::luma_counter(rmd::luma_bits(-0.0)) == 258u && rmd::luma_counter(rmd::luma_bits(-1.0)) == 259u &&
	           rmd::luma_counter(rmd::luma_bits(5e-324)) == 256u && rmd::luma_counter(rmd::luma_bits(inf)) == 260u && rmd::luma_counter(rmd::luma_bits(nan)) == 260u,
	       "the side counters");

	for (uint64_t it = 0; it < n_random; it++) {
		const uint32_t width = (uint32_t)(rng() % 41), height = (uint32_t)(rng() % 41), left = (uint32_t)(rng() % 4), top = (uint32_t)(rng() % 4);
		const uint32_t fw = left + width, fh = top + height; // the frame ends where the rect ends
		const uint32_t n = count_set[rng() % 5];
		const uint32_t table = (uint32_t)(rng() % 4); // 0: random (a fifth of the entries 0), 1: all zero, 2: all ones, 3: the tone curve's
		// scales: mostly where the bins are (2^-40 .. 2^40), the rest over 2^-500 .. 2^500
		const int scale = (rng() % 3) ? (int)(rng() % 81) - 40 : (int)(rng() % 1001) - 500;
		const uint32_t style = (uint32_t)(rng() % 4); // 0: clean positive, 1: a few specials, 2: many specials, 3: Q below S^2 / n (every variance clamps)
		std::vector<double> weights(rmd::kLumaWeights); // exactly 260 on the heap: a read of entry 260 is the sanitizer's
		if (table == 0)
			for (double &w : weights) w = (rng() % 5) ? std::ldexp(unit(rng), (int)(rng() % 41) - 20) : 0.0;
		else if (table == 2)
			for (double &w : weights) w = 1.0;
		else if (table == 3) {
			const double es[] = {1.0, 0.92, 1000.0, 0.001}, gs[] = {2.2, 1.0, 0.5};
			weights = display_table(es[rng() % 4], gs[rng() % 3], (rng() % 2) ? 1.0 / 255.0 : 0.1);
		}
		for (double w : weights) EXPECT(std::isfinite(w) && w >= 0.0, "rect %" PRIu64 ": a weight %.17g", it, w);
		std::vector<double> S((size_t)fw * fh * 3), Q((size_t)fw * fh * 3);
		for (size_t k = 0; k < S.size(); k++) {
			double s = std::ldexp(0.25 + unit(rng), scale), q = std::ldexp(0.25 + unit(rng), 2 * (scale > 250 ? 250 : scale < -250 ? -250 : scale));
			if (style == 3) q = 0.0;
			const uint32_t special = (uint32_t)(rng() % (style == 1 ? 400 : style == 2 ? 12 : 0x7FFFFFFF));
			switch (special) {
			case 0: s = 0.0; break;
			case 1: s = -0.0; break;
			case 2: s = -s; break;
			case 3: s = inf; break;
			case 4: s = -inf; break;
			case 5: s = nan; break;
			case 6: q = inf; break;
			case 7: q = nan; break;
			case 8: q = -q; break;
			case 9: q = -0.0; break;
			case 10: q = 1.7e308; break; // the largest V finite sums give
			default: break;
			}
			S[k] = s, Q[k] = q;
		}
		const rmd::TileWeighted got = rmd::tile_weighted_rect_host(S.data(), Q.data(), fw, left, top, width, height, n, weights.data());
		const rmd::TileWeighted want = plain_rect(S.data(), Q.data(), fw, left, top, width, height, n, weights);
		const uint64_t n_px = (uint64_t)width * height;
		rects++;
		EXPECT(same_bits(got.rms, want.rms) && same_bits(got.mean_weighted_variance, want.mean_weighted_variance) && same_bits(got.mean_luma, want.mean_luma) &&
		           same_bits(got.mean_variance, want.mean_variance) && got.valid == want.valid && got.invalid == want.invalid,
		       "rect %" PRIu64 " (%u x %u at count %u, table %u): %.17g %.17g %.17g %.17g %u %u against %.17g %.17g %.17g %.17g %u %u", it, width, height, n, table, got.rms,
		       got.mean_weighted_variance, got.mean_luma, got.mean_variance, got.valid, got.invalid, want.rms, want.mean_weighted_variance, want.mean_luma, want.mean_variance,
		       want.valid, want.invalid);
		EXPECT(!std::isnan(got.rms) && !std::isnan(got.mean_weighted_variance) && !std::isnan(got.mean_luma) && !std::isnan(got.mean_variance), "rect %" PRIu64 ": a NaN field", it);
		EXPECT((uint64_t)got.valid + got.invalid == n_px, "rect %" PRIu64 ": %u + %u pixels of %" PRIu64, it, got.valid, got.invalid, n_px);
		if (got.invalid) EXPECT(got.rms == inf, "rect %" PRIu64 ": %u invalid pixels, rms %.17g", it, got.invalid, got.rms);
		if (n < 2u) EXPECT(got.valid == 0u, "rect %" PRIu64 ": count %u, %u valid pixels", it, n, got.valid);
		if (n_px == 0)
			EXPECT(same_bits(got.rms, 0.0) && same_bits(got.mean_weighted_variance, 0.0) && same_bits(got.mean_luma, 0.0) && same_bits(got.mean_variance, 0.0) && got.valid == 0u &&
			           got.invalid == 0u,
			       "rect %" PRIu64 ": no pixels, not all zeros", it);
		EXPECT(got.mean_variance >= 0.0 && got.mean_weighted_variance >= 0.0 && got.rms >= 0.0, "rect %" PRIu64 ": a negative field", it);
		if (table == 1 && !got.invalid) EXPECT(same_bits(got.rms, 0.0) && same_bits(got.mean_weighted_variance, 0.0), "rect %" PRIu64 ": all-zero weights, rms %.17g", it, got.rms);
		if (table == 2) EXPECT(same_bits(got.mean_weighted_variance, got.mean_variance), "rect %" PRIu64 ": all-ones weights, %.17g against %.17g", it, got.mean_weighted_variance, got.mean_variance);
		if (n_px == 0) empty++;
		else if (got.invalid) with_invalid++;
		else {
			all_valid++;
			if (got.rms == 0.0) zero_rms++;
			if (got.rms == inf) infinite_valid++;
		}
	}

	// the per-pixel step on its edges: a zero weight gives +0 whatever V is
	{
		std::vector<double> weights(rmd::kLumaWeights, 0.0);
		weights[5] = 2.0, weights[259] = 0.5;
		EXPECT(same_bits(rmd::tile_weighted_pixel(inf, 0u, weights.data()), 0.0), "w = 0 under V = inf");
		EXPECT(same_bits(rmd::tile_weighted_pixel(3.0, 258u, weights.data()), 0.0), "w = 0 under V = 3");
		EXPECT(rmd::tile_weighted_pixel(3.0, 5u, weights.data()) == 6.0 && rmd::tile_weighted_pixel(inf, 5u, weights.data()) == inf, "w = 2");
		EXPECT(rmd::tile_weighted_pixel(4.0, 259u, weights.data()) == 2.0, "the last entry");
		rmd::TileWeightedSums a;
		const double s[3] = {8.0, 8.0, 8.0}, q[3] = {40.0, 40.0, 40.0}, bad[3] = {8.0, nan, 8.0};
		rmd::tile_weighted_add(a, s, q, 4u, weights.data());
		EXPECT(a.valid == 1u && a.invalid == 0u && a.sy > 1.99 && a.sy < 2.01 && a.sv > 0.0 && same_bits(a.se, 0.0), "a pixel at Y = 2 under a zero weight: %.17g %.17g %.17g", a.sy, a.sv, a.se);
		rmd::tile_weighted_add(a, bad, q, 4u, weights.data());
		rmd::tile_weighted_add(a, s, q, 1u, weights.data());
		EXPECT(a.valid == 1u && a.invalid == 2u && a.sy < 2.01, "a NaN sum and a count of 1");
	}
	// the final step: invalid pixels, overflowing sums
	{
		rmd::TileWeighted o = rmd::tile_weighted_final(8.0, 2.0, 18.0, 2u, 0u, 2u);
		EXPECT(o.mean_luma == 4.0 && o.mean_variance == 1.0 && o.mean_weighted_variance == 9.0 && o.rms == 3.0, "plain: %.17g", o.rms);
		o = rmd::tile_weighted_final(8.0, 2.0, 18.0, 2u, 1u, 3u);
		EXPECT(o.mean_luma == 4.0 && o.mean_variance == 1.0 && o.mean_weighted_variance == 9.0 && o.rms == inf && o.invalid == 1u, "one invalid: %.17g", o.rms);
		o = rmd::tile_weighted_final(0.0, 0.0, 0.0, 0u, 5u, 5u);
		EXPECT(o.mean_luma == 0.0 && o.mean_weighted_variance == 0.0 && o.rms == inf, "all invalid: %.17g", o.rms);
		o = rmd::tile_weighted_final(inf, inf, inf, 2u, 0u, 2u);
		EXPECT(o.rms == inf, "overflowing sums: %.17g", o.rms);
		o = rmd::tile_weighted_final(1.0, 1.0, nan, 2u, 0u, 2u);
		EXPECT(o.rms == inf, "a NaN rms is reported as +inf: %.17g", o.rms);
	}

	if (failures) {
		std::printf("%d failures\n", failures);
		return 1;
	}
	std::printf("tile weighted rule ok: %" PRIu64 " rects, %" PRIu64 " empty, %" PRIu64 " with an invalid pixel, %" PRIu64 " all valid, %" PRIu64 " of them with rms 0, %" PRIu64
	            " with an infinite rms\n",
	            rects, empty, with_invalid, all_valid, zero_rms, infinite_valid);
	return 0;
}
