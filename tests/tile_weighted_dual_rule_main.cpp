// Drives raymond_amd/csrc/tile_weighted_dual_rule.hpp — the rule of rmd_tile_weighted_error_dual, the lines its kernel is built from — on the CPU
// (tests/test_tile_weighted_dual_host.py builds this with -fsanitize=address,undefined and runs it directly).
//
//   tile_weighted_dual_rule <seed> <random rects>
//
// Every random rect — width and height 0 .. 40, filtered means and err with zeros of both signs, negatives, infinities and NaN among them at scales
// 2^-500 .. 2^500 (err: the square of that), on heap blocks that end exactly where the rect ends so that a read past them is the sanitizer's, under a
// weight table of exactly 260 heap doubles that is random, all zero, all ones or the tone curve's (rmd_display_weights' formula) — goes through
// tile_weighted_dual_rect_host and through a second plain reading below: the counter from comparisons and frexp instead of bits, an explicit array of
// 256 partials filled pixel by pixel, and an explicit tree.  The two must agree bit for bit.  Held as well: rms is never NaN; no field is NaN in a rect
// none of whose err is negative (sums of terms >= 0 cannot meet inf - inf; a rect with negative err beside +inf or overflow can, and err of the dual
// filters is never negative); invalid > 0 gives rms = +inf; valid + invalid is the rect's pixel count; a rect without pixels gives all zeros; an all-zero
// table gives rms 0 whatever err holds; and the per-pixel step adds 0 for w = 0 under e = +inf.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "tile_weighted_dual_rule.hpp"

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
// A pixel: validity, Y and E written out
static bool plain_pixel(const double *o, double e, const double *weights, double &Y, double &E) {
	if (std::isnan(e)) return false;
	for (int c = 0; c < 3; c++)
		if (!std::isfinite(o[c])) return false;
	const double y0 = 0.2126 * o[0], y1 = 0.7152 * o[1], y2 = 0.0722 * o[2];
	Y = (y0 + y1) + y2;
	const uint32_t k = plain_counter(Y);
	if (k >= 260u) return false;
	const double w = weights[k];
	E = w == 0.0 ? 0.0 : w * e;
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
static rmd::TileWeighted plain_rect(const double *out, const double *err, uint32_t frame_width, uint32_t left, uint32_t top, uint32_t width, uint32_t height,
                                    const double *weights) {
	double py[256] = {}, pv[256] = {}, pe[256] = {};
	uint32_t valid[256] = {}, invalid[256] = {};
	uint64_t i = 0;
	for (uint32_t y = 0; y < height; y++)
		for (uint32_t x = 0; x < width; x++, i++) { // row-major within the rect: pixel i belongs to lane i % 256, which meets its pixels in ascending i
			const size_t pix = (size_t)(left + x) + (size_t)(top + y) * frame_width;
			double Y, E;
			if (plain_pixel(out + pix * 3, err[pix], weights, Y, E)) py[i % 256] += Y, pv[i % 256] += err[pix], pe[i % 256] += E, valid[i % 256]++;
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
static void display_table(double e, double g, double floor, double *out) {
	const double y_floor = -std::log1p(-std::pow(floor, g)) / e;
	auto weight = [&](double y) {
		const double t = -std::expm1(-y * e), slope = (1.0 / g) * std::pow(t, 1.0 / g - 1.0) * e * std::exp(-y * e), w = slope * slope;
		return std::isnan(w) ? 0.0 : w > std::numeric_limits<double>::max() ? std::numeric_limits<double>::max() : w;
	};
	for (uint32_t i = 0; i < 256u; i++) {
		const double y = std::ldexp(1.0 + ((double)(i % 4u) + 0.5) * 0.25, (int)(i / 4u) - 32);
		out[i] = weight(y > y_floor ? y : y_floor);
	}
	out[256] = out[258] = out[259] = weight(y_floor);
	out[257] = weight(std::ldexp(1.0, 32));
}

int main(int argc, char **argv) {
	const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
	const uint64_t n_random = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 10000;
	std::mt19937_64 rng(seed);
	const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
	std::uniform_real_distribution<double> unit(0.0, 1.0);
	uint64_t rects = 0, empty = 0, with_invalid = 0, all_valid = 0, zero_rms = 0, infinite_valid = 0, guarded = 0;

	for (uint64_t it = 0; it < n_random; it++) {
		const uint32_t width = (uint32_t)(rng() % 41), height = (uint32_t)(rng() % 41), left = (uint32_t)(rng() % 4), top = (uint32_t)(rng() % 4);
		const uint32_t fw = left + width, fh = top + height; // the frame ends where the rect ends
		const uint32_t table = (uint32_t)(rng() % 4); // 0: random (a fifth of the entries 0), 1: all zero, 2: all ones, 3: the tone curve's
		// scales: mostly where the bins are (2^-40 .. 2^40), the rest over 2^-500 .. 2^500
		const int scale = (rng() % 3) ? (int)(rng() % 81) - 40 : (int)(rng() % 1001) - 500;
		const uint32_t style = (uint32_t)(rng() % 3); // 0: clean positive, 1: a few specials, 2: many specials
		std::unique_ptr<double[]> weights(new double[rmd::kLumaWeights]()); // exactly 260 on the heap: a read of entry 260 is the sanitizer's
		if (table == 0)
			for (uint32_t k = 0; k < rmd::kLumaWeights; k++) weights[k] = (rng() % 5) ? std::ldexp(unit(rng), (int)(rng() % 41) - 20) : 0.0;
		else if (table == 2)
			for (uint32_t k = 0; k < rmd::kLumaWeights; k++) weights[k] = 1.0;
		else if (table == 3) {
			const double es[] = {1.0, 0.92, 1000.0, 0.001}, gs[] = {2.2, 1.0, 0.5};
			display_table(es[rng() % 4], gs[rng() % 3], (rng() % 2) ? 1.0 / 255.0 : 0.1, weights.get());
		}
		for (uint32_t k = 0; k < rmd::kLumaWeights; k++) EXPECT(std::isfinite(weights[k]) && weights[k] >= 0.0, "rect %" PRIu64 ": a weight %.17g", it, weights[k]);
		const size_t n_frame = (size_t)fw * fh;
		std::unique_ptr<double[]> out(new double[n_frame * 3]), err(new double[n_frame]); // exact-size heap blocks
		bool negative_err = false, infinite_err_under_zero = false;
		const auto special_count = style == 1 ? 400u : style == 2 ? 12u : 0x7FFFFFFFu;
		for (size_t p = 0; p < n_frame; p++) {
			for (int c = 0; c < 3; c++) {
				double o = std::ldexp(0.25 + unit(rng), scale);
				switch ((uint32_t)(rng() % special_count)) {
				case 0: o = 0.0; break;
				case 1: o = -0.0; break;
				case 2: o = -o; break;
				case 3: o = inf; break;
				case 4: o = -inf; break;
				case 5: o = nan; break;
				default: break;
				}
				out[p * 3 + c] = o;
			}
			double e = std::ldexp(0.25 + unit(rng), 2 * scale);
			switch ((uint32_t)(rng() % special_count)) {
			case 0: e = 0.0; break;
			case 1: e = -0.0; break;
			case 2: e = -e; break;
			case 3:
			case 4: e = inf; break;
			case 5: e = nan; break;
			case 6: e = -inf; break;
			default: break;
			}
			err[p] = e;
		}
		for (uint32_t y = 0; y < height; y++)
			for (uint32_t x = 0; x < width; x++) {
				const size_t pix = (size_t)(left + x) + (size_t)(top + y) * fw;
				if (err[pix] < 0.0) negative_err = true;
				double Y, E;
				if (err[pix] == inf && plain_pixel(&out[pix * 3], err[pix], weights.get(), Y, E) && E == 0.0) infinite_err_under_zero = true;
			}
		const rmd::TileWeighted got = rmd::tile_weighted_dual_rect_host(out.get(), err.get(), fw, left, top, width, height, weights.get());
		const rmd::TileWeighted want = plain_rect(out.get(), err.get(), fw, left, top, width, height, weights.get());
		const uint64_t n_px = (uint64_t)width * height;
		rects++;
		EXPECT(same_bits(got.rms, want.rms) && same_bits(got.mean_weighted_variance, want.mean_weighted_variance) && same_bits(got.mean_luma, want.mean_luma) &&
		           same_bits(got.mean_variance, want.mean_variance) && got.valid == want.valid && got.invalid == want.invalid,
		       "rect %" PRIu64 " (%u x %u, table %u): %.17g %.17g %.17g %.17g %u %u against %.17g %.17g %.17g %.17g %u %u", it, width, height, table, got.rms,
		       got.mean_weighted_variance, got.mean_luma, got.mean_variance, got.valid, got.invalid, want.rms, want.mean_weighted_variance, want.mean_luma, want.mean_variance,
		       want.valid, want.invalid);
		EXPECT(!std::isnan(got.rms) && !std::isnan(got.mean_luma), "rect %" PRIu64 ": a NaN rms or mean_luma", it);
		if (!negative_err) EXPECT(!std::isnan(got.mean_weighted_variance) && !std::isnan(got.mean_variance), "rect %" PRIu64 ": a NaN field without a negative err", it);
		EXPECT((uint64_t)got.valid + got.invalid == n_px, "rect %" PRIu64 ": %u + %u pixels of %" PRIu64, it, got.valid, got.invalid, n_px);
		if (got.invalid) EXPECT(got.rms == inf, "rect %" PRIu64 ": %u invalid pixels, rms %.17g", it, got.invalid, got.rms);
		if (n_px == 0)
			EXPECT(same_bits(got.rms, 0.0) && same_bits(got.mean_weighted_variance, 0.0) && same_bits(got.mean_luma, 0.0) && same_bits(got.mean_variance, 0.0) && got.valid == 0u &&
			           got.invalid == 0u,
			       "rect %" PRIu64 ": no pixels, not all zeros", it);
		if (table == 1 && !got.invalid) EXPECT(same_bits(got.rms, 0.0) && same_bits(got.mean_weighted_variance, 0.0), "rect %" PRIu64 ": all-zero weights, rms %.17g", it, got.rms);
		if (table == 2 && !std::isnan(got.mean_variance))
			EXPECT(same_bits(got.mean_weighted_variance, got.mean_variance), "rect %" PRIu64 ": all-ones weights, %.17g against %.17g", it, got.mean_weighted_variance, got.mean_variance);
		if (infinite_err_under_zero) guarded++;
		if (n_px == 0) empty++;
		else if (got.invalid) with_invalid++;
		else {
			all_valid++;
			if (got.rms == 0.0) zero_rms++;
			if (got.rms == inf) infinite_valid++;
		}
	}

	// the per-pixel step on its edges: w = 0 under e = +inf adds 0, and the pixel is valid
	{
		std::unique_ptr<double[]> weights(new double[rmd::kLumaWeights]());
		weights[5] = 2.0, weights[259] = 0.5;
		const double grey[3] = {2.0, 2.0, 2.0}, dark[3] = {-1.0, -1.0, -1.0}, bad[3] = {2.0, nan, 2.0}, inf_mean[3] = {2.0, 2.0, -inf};
		rmd::TileSums a;
		rmd::tile_weighted_dual_add(a, grey, inf, weights.get()); // Y = 2: bin 132, weight 0
		EXPECT(a.valid == 1u && a.invalid == 0u && a.sy > 1.99 && a.sy < 2.01 && a.sv == inf && same_bits(a.se, 0.0), "w = 0 under e = inf: %.17g %.17g %.17g", a.sy, a.sv, a.se);
		rmd::TileSums b;
		rmd::tile_weighted_dual_add(b, dark, 4.0, weights.get()); // Y < 0: the last entry
		rmd::tile_weighted_dual_add(b, dark, -4.0, weights.get()); // a negative err is added as it is
		EXPECT(b.valid == 2u && same_bits(b.se, 0.0) && same_bits(b.sv, 0.0) && b.sy < -1.99, "the last entry, and a negative err: %.17g %.17g", b.sv, b.se);
		rmd::tile_weighted_dual_add(b, bad, 1.0, weights.get());
		rmd::tile_weighted_dual_add(b, grey, nan, weights.get());
		rmd::tile_weighted_dual_add(b, inf_mean, 1.0, weights.get());
		EXPECT(b.valid == 2u && b.invalid == 3u, "a NaN mean, a NaN err and an infinite mean: %u %u", b.valid, b.invalid);
	}

	if (failures) {
		std::printf("%d failures\n", failures);
		return 1;
	}
	std::printf("tile weighted dual rule ok: %" PRIu64 " rects, %" PRIu64 " empty, %" PRIu64 " with an invalid pixel, %" PRIu64 " all valid, %" PRIu64 " of them with rms 0, %" PRIu64
	            " with an infinite rms, %" PRIu64 " with w = 0 under e = inf\n",
	            rects, empty, with_invalid, all_valid, zero_rms, infinite_valid, guarded);
	return 0;
}
