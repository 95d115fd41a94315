// Drives raymond_amd/csrc/despike_rule.hpp — the rule of rmd_despike, the lines its kernel is built from — on the CPU
// (tests/test_despike_host.py builds this with -fsanitize=address,undefined and runs it directly).
//
//   despike_rule <seed> <random windows>
//
// Every random window — radius 1 .. 3, a rank over the whole legal range, luminances drawn from a handful of values so that ties abound, with NaN marks
// (no other), negatives, zeros of both signs and infinities among them, in a row stride wider than the window — is held against a straightforward reading:
// the others collected into a vector and std::stable_sort-ed by luminance descending, which keeps the raster order among equals.  Checked per window: the
// donor (despike_donor), the count the shortcut takes (despike_at_or_above), and that despike_settled never settles a pixel the full rule calls a spike —
// at ratios and floors drawn with it.  Then the argument edges: rank at its maximum in a full window and in a corner's, windows without others, k = 0,
// ratio = 1, floor = 0 on equality, NaN and infinite V, the scaled copy, and Y and V against the products and additions written out.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "despike_rule.hpp"

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

struct Other {
	double y;
	uint32_t i;
};

// The donor by sorting: -1 with fewer than rank + 1 others
static int donor_by_sort(const std::vector<double> &win, uint32_t stride, uint32_t radius, uint32_t rank) {
	const uint32_t side = 2 * radius + 1;
	std::vector<Other> others;
	for (uint32_t row = 0; row < side; row++)
		for (uint32_t col = 0; col < side; col++) {
			const double y = win[row * stride + col];
			if ((row == radius && col == radius) || std::isnan(y)) continue;
			others.push_back(Other{y, row * side + col});
		}
	std::stable_sort(others.begin(), others.end(), [](const Other &a, const Other &b) { return a.y > b.y; });
	return rank < others.size() ? (int)others[rank].i : -1;
}

int main(int argc, char **argv) {
	const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
	const uint64_t n_random = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 100000;
	std::mt19937_64 rng(seed);
	const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
	const double palette[] = {0.0, -0.0, 1.0, 1.0, 1.0, 2.5, 2.5, 50.0, -1.0, -1.0, -3.5, 1e-300, -1e-300, 1e300, inf, -inf, 0.75, 0.75};
	const size_t n_palette = sizeof(palette) / sizeof(palette[0]);
	uint64_t windows = 0, with_ties = 0, without_donor = 0, settled = 0, spikes = 0, negative_spikes = 0;

	for (uint64_t it = 0; it < n_random; it++) {
		const uint32_t radius = 1 + (uint32_t)(rng() % rmd::kDespikeMaxRadius), side = 2 * radius + 1, stride = side + (uint32_t)(rng() % 5);
		const uint32_t rank = (uint32_t)(rng() % (side * side - 1));
		std::vector<double> win((size_t)(side - 1) * stride + side, nan); // exactly the doubles a window spans: a read past either end is the sanitizer's
		const uint32_t style = (uint32_t)(rng() % 4); // 0: mostly ties, 1: random doubles, 2: many NaN marks, 3: negatives only
		for (uint32_t row = 0; row < side; row++)
			for (uint32_t col = 0; col < side; col++) {
				double y;
				if (style == 1) y = std::ldexp((double)(int64_t)(rng() % 2001) - 1000.0, (int)(rng() % 7) - 3);
				else if (style == 3) y = -palette[2 + rng() % 6];
				else y = palette[rng() % n_palette];
				if (rng() % (style == 2 ? 2 : 9) == 0) y = nan;
				win[row * stride + col] = y;
			}
		double &centre = win[radius * stride + radius];
		if (std::isnan(centre)) centre = palette[rng() % n_palette]; // p itself is valid: its Y is never NaN
		const double yp = centre;
		windows++;

		const int want = donor_by_sort(win, stride, radius, rank), got = rmd::despike_donor(win.data(), stride, radius, rank);
		EXPECT(want == got, "window %" PRIu64 ": radius %u rank %u, donor %d by sorting, %d by the header", it, radius, rank, want, got);
		if (want < 0) without_donor++;

		uint32_t at_or_above = 0, ties = 0;
		for (uint32_t row = 0; row < side; row++)
			for (uint32_t col = 0; col < side; col++) {
				if (row == radius && col == radius) continue;
				const double y = win[row * stride + col];
				if (y >= yp) at_or_above++;
				if (y == yp) ties++;
			}
		if (ties) with_ties++;
		EXPECT(at_or_above == rmd::despike_at_or_above(win.data(), stride, radius, yp), "window %" PRIu64 ": the count at or above", it);

		// the shortcut never hides a spike: whenever it settles a pixel, the full rule says "no spike" at every legal ratio and floor
		const double ratios[] = {1.0, 1.5, 2.0, 1e6}, floors[] = {0.0, 0.25, 1e300}, ks[] = {0.0, 6.0};
		const bool is_settled = rmd::despike_settled(at_or_above, rank, yp);
		if (is_settled) settled++;
		if (want >= 0) {
			const double yd = win[(uint32_t)want / side * stride + (uint32_t)want % side];
			for (double ratio : ratios)
				for (double floor : floors)
					for (double k : ks) {
						const bool spike = rmd::despike_is_spike(yp, yd, 0.01, k, ratio, floor);
						const double e = (yp - ratio * yd) - floor;
						EXPECT(spike == (e > 0.0 && e * e > (k * k) * 0.01), "window %" PRIu64 ": the test written out", it);
						if (is_settled) EXPECT(!spike, "window %" PRIu64 ": settled by the count (%u at or above, rank %u, Y_p %g, Y_q* %g) but a spike at ratio %g", it, at_or_above, rank, yp, yd, ratio);
						if (spike) spikes++;
						if (spike && yd < 0.0 && at_or_above > rank) negative_spikes++; // what a count that forgot the sign would have dropped
					}
		} else EXPECT(!is_settled, "window %" PRIu64 ": settled without a donor", it);
	}

	// ---- the edges
	for (uint32_t radius = 1; radius <= rmd::kDespikeMaxRadius; radius++) {
		const uint32_t side = 2 * radius + 1, n = side * side, max_rank = n - 2;
		std::vector<double> win(n);
		for (uint32_t i = 0; i < n; i++) win[i] = (double)i; // the last offset is the brightest
		win[n / 2] = 1e9;                                    // p itself is skipped, however bright
		EXPECT(rmd::despike_donor(win.data(), side, radius, 0) == (int)n - 1, "rank 0 takes the brightest other");
		EXPECT(rmd::despike_donor(win.data(), side, radius, max_rank) == 0, "the largest rank takes the darkest other of a full window");
		EXPECT(rmd::despike_donor(win.data(), side, radius, max_rank + 1) == -1, "one more has no donor");
		std::fill(win.begin(), win.end(), 1.0); // all ties: the order is the raster order, the centre left out
		for (uint32_t rank = 0; rank <= max_rank; rank++)
			EXPECT(rmd::despike_donor(win.data(), side, radius, rank) == (int)(rank < n / 2 ? rank : rank + 1), "ties go by raster order (radius %u rank %u)", radius, rank);
		// a corner pixel's window: only the lower right quarter holds others
		for (uint32_t row = 0; row < side; row++)
			for (uint32_t col = 0; col < side; col++)
				if (row < radius || col < radius) win[row * side + col] = nan;
		const uint32_t in_corner = (radius + 1) * (radius + 1) - 1;
		EXPECT(rmd::despike_donor(win.data(), side, radius, in_corner - 1) >= 0 && rmd::despike_donor(win.data(), side, radius, in_corner) == -1, "a corner has %u others", in_corner);
		std::fill(win.begin(), win.end(), nan);
		win[n / 2] = 5.0;
		EXPECT(rmd::despike_donor(win.data(), side, radius, 0) == -1 && rmd::despike_at_or_above(win.data(), side, radius, 5.0) == 0, "a window without others");
		EXPECT(rmd::despike_raster(-(int)radius, -(int)radius, radius) == 0 && rmd::despike_raster((int)radius, (int)radius, radius) == n - 1 &&
		           rmd::despike_raster(0, 0, radius) == n / 2, "the raster index of an offset");
	}
	EXPECT(!rmd::despike_is_spike(1.0, 1.0, 1e-6, 0.0, 1.0, 0.0), "equality at ratio 1, k 0, floor 0 is no spike: e > 0 fails");
	EXPECT(rmd::despike_is_spike(std::nextafter(1.0, 2.0), 1.0, 0.0, 0.0, 1.0, 0.0), "one ulp above it is, at k 0 with V 0: e * e > 0");
	EXPECT(!rmd::despike_is_spike(50.0, 1.0, nan, 6.0, 2.0, 0.0) && !rmd::despike_is_spike(50.0, 1.0, inf, 6.0, 2.0, 0.0), "a NaN or infinite V makes no spike");
	EXPECT(rmd::despike_is_spike(50.0, 1.0, inf, 0.0, 2.0, 0.0) == false, "k 0 with an infinite V: 0 * inf is NaN, no spike");
	EXPECT(!rmd::despike_is_spike(inf, inf, 0.0, 6.0, 2.0, 0.0), "inf - inf is NaN: no spike");
	EXPECT(!rmd::despike_is_spike(50.0, 1.0, 1e-6, 6.0, 2.0, 1e300), "a floor above every spike");
	EXPECT(rmd::despike_is_spike(-1.5, -1.0, 1e-6, 6.0, 2.0, 0.0), "a negative donor: e = -1.5 + 2 > 0");
	EXPECT(!rmd::despike_settled(24, 2, -1.5) && rmd::despike_settled(3, 2, 0.0) && rmd::despike_settled(3, 2, -0.0) && !rmd::despike_settled(2, 2, 1.0), "what the count settles");
	EXPECT(rmd::despike_scaled(10.0, 5, 16) == (10.0 / 5.0) * 16.0 && rmd::despike_scaled(1.0, 3, 7) == (1.0 / 3.0) * 7.0, "the scaled copy");
	{
		volatile double pr = 0.2126 * 0.3, pg = 0.7152 * 0.6, pb = 0.0722 * 0.9;
		volatile double sum = pr + pg;
		EXPECT(rmd::despike_luma(0.3, 0.6, 0.9) == sum + pb, "Y");
		volatile double a0 = 0.2126 * 0.2126, a1 = 0.7152 * 0.7152, a2 = 0.0722 * 0.0722;
		volatile double q0 = a0 * 0.3, q1 = a1 * 0.6, q2 = a2 * 0.9;
		volatile double qs = q0 + q1;
		EXPECT(rmd::despike_luma_variance(0.3, 0.6, 0.9) == qs + q2, "V");
		const double s[3] = {16.0, 32.0, 8.0}, q[3] = {17.0, 70.0, 5.0}, bad[3] = {16.0, nan, 8.0}, big[3] = {16.0, inf, 8.0};
		double Y = 0, V = 0;
		EXPECT(rmd::despike_pixel(s, q, 16, Y, V) && Y == rmd::despike_luma(1.0, 2.0, 0.5) && V > 0.0, "a valid pixel");
		EXPECT(!rmd::despike_pixel(s, q, 1, Y, V) && !rmd::despike_pixel(s, q, 0, Y, V) && !rmd::despike_pixel(bad, q, 16, Y, V) && !rmd::despike_pixel(s, big, 16, Y, V) &&
		           !rmd::despike_pixel(s, bad, 16, Y, V), "count below 2, NaN and inf sums are not valid");
		double u = 0, v = 0;
		rmd::despike_moments(16.0, 1.0, 16.0, u, v); // Q below S * u: the variance is clamped
		EXPECT(u == 1.0 && v == 0.0 && !std::signbit(v), "max(0, .)");
	}
	std::printf("despike rule %s: %" PRIu64 " windows, %" PRIu64 " with ties, %" PRIu64 " without a donor, %" PRIu64 " settled by the count, %" PRIu64
	            " spikes, %" PRIu64 " of them under a negative donor with more than rank others at or above\n",
	            failures ? "FAILED" : "ok", windows, with_ties, without_donor, settled, spikes, negative_spikes);
	return failures ? 1 : 0;
}
