// Drives raymond_amd/csrc/tile_luma_rule.hpp — the rule of rmd_tile_luma_error, the lines its kernel is built from — on the CPU
// (tests/test_tile_luma_host.py builds this with -fsanitize=address,undefined and runs it directly).
//
//   tile_luma_rule <seed> <random rects>
//
// Every random rect — width and height 0 .. 40, a count from {0, 1, 2, 3, 2^32 - 1}, sums with zeros of both signs, negatives, infinities and NaN among
// them at scales 2^-500 .. 2^500, in a frame that ends exactly where the rect ends so that a read past it is the sanitizer's — goes through
// tile_luma_rect_host and through a second plain reading below: the arithmetic of a pixel written out, an explicit array of 256 partials filled pixel by
// pixel, and an explicit tree.  The two must agree bit for bit.  Held as well: no field is NaN; invalid > 0 gives +inf errors; valid + invalid is the
// rect's pixel count; a rect without pixels gives all zeros; a count below 2 makes every pixel invalid.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "tile_luma_rule.hpp"

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

// The second reading.  A pixel: validity, Y, V and R written out
static bool plain_pixel(const double *s, const double *q, uint32_t n, double floor, double &Y, double &V, double &R) {
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
	const double d = std::fabs(Y) > floor ? std::fabs(Y) : floor;
	const double vd = V / d;
	R = vd / d;
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
static rmd::TileLuma plain_rect(const double *S, const double *Q, uint32_t frame_width, uint32_t left, uint32_t top, uint32_t width, uint32_t height, uint32_t n, double floor) {
	double py[256] = {}, pv[256] = {}, pr[256] = {};
	uint32_t valid[256] = {}, invalid[256] = {};
	uint64_t i = 0;
	for (uint32_t y = 0; y < height; y++)
		for (uint32_t x = 0; x < width; x++, i++) { // row-major within the rect: pixel i belongs to lane i % 256, which meets its pixels in ascending i
			const size_t pix = (size_t)(left + x) + (size_t)(top + y) * frame_width;
			double Y, V, R;
			if (plain_pixel(S + pix * 3, Q + pix * 3, n, floor, Y, V, R)) py[i % 256] += Y, pv[i % 256] += V, pr[i % 256] += R, valid[i % 256]++;
			else invalid[i % 256]++;
		}
	const double inf = std::numeric_limits<double>::infinity();
	rmd::TileLuma o{};
	o.valid = plain_tree(valid), o.invalid = plain_tree(invalid);
	if (i == 0) return o;
	const double SY = plain_tree(py), SV = plain_tree(pv), SR = plain_tree(pr), m = (double)o.valid;
	o.mean_luma = o.valid ? SY / m : 0.0, o.mean_variance = o.valid ? SV / m : 0.0, o.mean_rel_variance = o.valid ? SR / m : 0.0;
	const double D = std::fabs(o.mean_luma) > floor ? std::fabs(o.mean_luma) : floor;
	o.tile_rms = std::sqrt(o.mean_variance) / D, o.pixel_rms = std::sqrt(o.mean_rel_variance);
	if (o.invalid) o.tile_rms = o.pixel_rms = inf;
	if (std::isnan(o.tile_rms)) o.tile_rms = inf;
	if (std::isnan(o.pixel_rms)) o.pixel_rms = inf;
	return o;
}

int main(int argc, char **argv) {
	const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
	const uint64_t n_random = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 10000;
	std::mt19937_64 rng(seed);
	const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
	const uint32_t count_set[] = {0u, 1u, 2u, 3u, 0xFFFFFFFFu};
	const double floors[] = {1e-3, 1.0, std::ldexp(1.0, -600), std::ldexp(1.0, 400)};
	std::uniform_real_distribution<double> unit(0.0, 1.0);
	uint64_t rects = 0, empty = 0, with_invalid = 0, all_valid = 0, clamped = 0, infinite_valid = 0;

	for (uint64_t it = 0; it < n_random; it++) {
		const uint32_t width = (uint32_t)(rng() % 41), height = (uint32_t)(rng() % 41), left = (uint32_t)(rng() % 4), top = (uint32_t)(rng() % 4);
		const uint32_t fw = left + width, fh = top + height; // the frame ends where the rect ends
		const uint32_t n = count_set[rng() % 5];
		const double floor = floors[rng() % 4];
		const int scale = (int)(rng() % 1001) - 500;
		const uint32_t style = (uint32_t)(rng() % 4); // 0: clean positive, 1: a few specials, 2: many specials, 3: Q below S^2 / n (every variance clamps)
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
			default: break;
			}
			S[k] = s, Q[k] = q;
		}
		const rmd::TileLuma got = rmd::tile_luma_rect_host(S.data(), Q.data(), fw, left, top, width, height, n, floor);
		const rmd::TileLuma want = plain_rect(S.data(), Q.data(), fw, left, top, width, height, n, floor);
		const uint64_t n_px = (uint64_t)width * height;
		rects++;
		EXPECT(same_bits(got.tile_rms, want.tile_rms) && same_bits(got.pixel_rms, want.pixel_rms) && same_bits(got.mean_luma, want.mean_luma) &&
		           same_bits(got.mean_variance, want.mean_variance) && same_bits(got.mean_rel_variance, want.mean_rel_variance) && got.valid == want.valid &&
		           got.invalid == want.invalid,
		       "rect %" PRIu64 " (%u x %u at count %u): %.17g %.17g %.17g %.17g %.17g %u %u against %.17g %.17g %.17g %.17g %.17g %u %u", it, width, height, n, got.tile_rms,
		       got.pixel_rms, got.mean_luma, got.mean_variance, got.mean_rel_variance, got.valid, got.invalid, want.tile_rms, want.pixel_rms, want.mean_luma,
		       want.mean_variance, want.mean_rel_variance, want.valid, want.invalid);
		EXPECT(!std::isnan(got.tile_rms) && !std::isnan(got.pixel_rms) && !std::isnan(got.mean_luma) && !std::isnan(got.mean_variance) && !std::isnan(got.mean_rel_variance),
		       "rect %" PRIu64 ": a NaN field", it);
		EXPECT((uint64_t)got.valid + got.invalid == n_px, "rect %" PRIu64 ": %u + %u pixels of %" PRIu64, it, got.valid, got.invalid, n_px);
		if (got.invalid) EXPECT(got.tile_rms == inf && got.pixel_rms == inf, "rect %" PRIu64 ": %u invalid pixels, errors %.17g %.17g", it, got.invalid, got.tile_rms, got.pixel_rms);
		if (n < 2u) EXPECT(got.valid == 0u, "rect %" PRIu64 ": count %u, %u valid pixels", it, n, got.valid);
		if (n_px == 0)
			EXPECT(same_bits(got.tile_rms, 0.0) && same_bits(got.pixel_rms, 0.0) && same_bits(got.mean_luma, 0.0) && same_bits(got.mean_variance, 0.0) &&
			           same_bits(got.mean_rel_variance, 0.0) && got.valid == 0u && got.invalid == 0u,
			       "rect %" PRIu64 ": no pixels, not all zeros", it);
		EXPECT(got.mean_variance >= 0.0 && got.mean_rel_variance >= 0.0 && got.tile_rms >= 0.0 && got.pixel_rms >= 0.0, "rect %" PRIu64 ": a negative field", it);
		if (n_px == 0) empty++;
		else if (got.invalid) with_invalid++;
		else {
			all_valid++;
			if (got.mean_variance == 0.0) clamped++;
			if (got.tile_rms == inf || got.pixel_rms == inf) infinite_valid++;
		}
	}

	// the per-pixel step on its edges: the floor takes over at and below it and for a zero of either sign; two divisions
	{
		double d, R;
		rmd::tile_luma_pixel(0.0, 4.0, 0.5, d, R);
		EXPECT(d == 0.5 && R == 16.0, "Y = 0: d %.17g R %.17g", d, R);
		rmd::tile_luma_pixel(-0.0, 4.0, 0.5, d, R);
		EXPECT(d == 0.5 && R == 16.0, "Y = -0: d %.17g R %.17g", d, R);
		rmd::tile_luma_pixel(-2.0, 4.0, 0.5, d, R);
		EXPECT(d == 2.0 && R == 1.0, "Y = -2: d %.17g R %.17g", d, R);
		rmd::tile_luma_pixel(0.5, 1.0, 0.5, d, R);
		EXPECT(d == 0.5 && R == 4.0, "Y = floor: d %.17g R %.17g", d, R);
		rmd::tile_luma_pixel(3.0, inf, 0.5, d, R);
		EXPECT(d == 3.0 && R == inf, "V = inf: d %.17g R %.17g", d, R);
		const double big = std::ldexp(1.0, 600), V = std::ldexp(1.0, 1000);
		rmd::tile_luma_pixel(big, V, 0.5, d, R); // d * d would overflow: (V / d) / d does not
		EXPECT(R == std::ldexp(1.0, -200), "(V / d) / d at d = 2^600: %.17g", R);
	}
	// the final step: invalid pixels, overflowing sums, the floor under the tile's mean
	{
		rmd::TileLuma o = rmd::tile_luma_final(8.0, 2.0, 18.0, 2u, 0u, 2u, 1e-3);
		EXPECT(o.mean_luma == 4.0 && o.mean_variance == 1.0 && o.mean_rel_variance == 9.0 && o.tile_rms == 0.25 && o.pixel_rms == 3.0, "plain: %.17g %.17g", o.tile_rms, o.pixel_rms);
		o = rmd::tile_luma_final(8.0, 2.0, 18.0, 2u, 1u, 3u, 1e-3);
		EXPECT(o.mean_luma == 4.0 && o.mean_variance == 1.0 && o.tile_rms == inf && o.pixel_rms == inf && o.invalid == 1u, "one invalid: %.17g %.17g", o.tile_rms, o.pixel_rms);
		o = rmd::tile_luma_final(0.0, 0.0, 0.0, 0u, 5u, 5u, 1e-3);
		EXPECT(o.mean_luma == 0.0 && o.tile_rms == inf && o.pixel_rms == inf, "all invalid: %.17g %.17g", o.tile_rms, o.pixel_rms);
		o = rmd::tile_luma_final(inf, inf, inf, 2u, 0u, 2u, 1e-3);
		EXPECT(o.tile_rms == inf && o.pixel_rms == inf, "inf / inf: %.17g %.17g", o.tile_rms, o.pixel_rms);
		o = rmd::tile_luma_final(-1e-6, 2.0, 2.0, 2u, 0u, 2u, 0.5);
		EXPECT(o.tile_rms == 2.0, "the floor under the mean: %.17g", o.tile_rms);
	}

	if (failures) {
		std::printf("%d failures\n", failures);
		return 1;
	}
	std::printf("tile luma rule ok: %" PRIu64 " rects, %" PRIu64 " empty, %" PRIu64 " with an invalid pixel, %" PRIu64 " all valid, %" PRIu64 " of them with every variance clamped, %" PRIu64
	            " with an infinite error\n",
	            rects, empty, with_invalid, all_valid, clamped, infinite_valid);
	return 0;
}
