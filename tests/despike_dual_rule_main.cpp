// Drives raymond_amd/csrc/despike_dual_rule.hpp — what rmd_despike_dual adds to the rule of rmd_despike, the lines its kernel is built from — on the CPU
// (tests/test_despike_dual_host.py builds this with -fsanitize=address,undefined and runs it directly).
//
//   despike_dual_rule <seed> <random windows>
//
// Every random window — radius 1 .. 3, a rank over the whole legal range, each position two halves of six sums and a count, drawn so that ties, empty
// halves, NaN and infinities in one half only, halves whose sum overflows, negatives and zeros of both signs abound — lies in heap blocks of exactly the
// window's size, so a read past either end is the sanitizer's.  The centre's twelve output values are made twice: through the headers the way the kernel
// drives them (despike_dual_pixel into a Y / V window, despike_donor, despike_is_spike, despike_dual_take), and by a second plain reading: the merge written
// out, std::isfinite, the moments written out, the others sorted with std::stable_sort, the copy written out.  The two must agree bit for bit.  Then the edges.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "despike_dual_rule.hpp"

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

static uint64_t bits(double x) {
	uint64_t b;
	std::memcpy(&b, &x, sizeof b);
	return b;
}

struct Other {
	double y;
	uint32_t i;
};

// The plain reading of one merged pixel: false when it is not valid
static bool plain_pixel(const double *sa, const double *qa, uint32_t na, const double *sb, const double *qb, uint32_t nb, double &Y, double &V) {
	if (na < 1 || nb < 1) return false;
	volatile double s[3], q[3];
	for (int c = 0; c < 3; c++) {
		s[c] = sa[c] + sb[c], q[c] = qa[c] + qb[c];
		if (!std::isfinite(s[c]) || !std::isfinite(q[c])) return false;
	}
	const double nd = (double)((uint64_t)na + nb);
	volatile double u[3], v[3];
	for (int c = 0; c < 3; c++) {
		u[c] = s[c] / nd;
		volatile double su = s[c] * u[c];
		volatile double t = (q[c] - su) / (nd - 1.0);
		if (!(t > 0.0)) t = 0.0;
		v[c] = t / nd;
	}
	volatile double yr = 0.2126 * u[0], yg = 0.7152 * u[1], yb = 0.0722 * u[2];
	volatile double yrg = yr + yg;
	Y = yrg + yb;
	volatile double a0 = 0.2126 * 0.2126, a1 = 0.7152 * 0.7152, a2 = 0.0722 * 0.0722;
	volatile double p0 = a0 * v[0], p1 = a1 * v[1], p2 = a2 * v[2];
	volatile double p01 = p0 + p1;
	V = p01 + p2;
	return true;
}

int main(int argc, char **argv) {
	const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
	const uint64_t n_random = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 100000;
	std::mt19937_64 rng(seed);
	const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
	const double means[] = {0.0, -0.0, 1.0, 1.0, 1.0, 2.5, 2.5, 50.0, -1.0, -3.5, 0.75, 0.75, 400.0};
	const uint32_t counts[] = {0, 1, 1, 8, 8, 8, 16, 16, 5};
	uint64_t windows = 0, centre_invalid = 0, without_donor = 0, spikes = 0, scaled_one_half = 0, scaled_both = 0, copied_both = 0, empty_half_others = 0;

	for (uint64_t it = 0; it < n_random; it++) {
		const uint32_t radius = 1 + (uint32_t)(rng() % rmd::kDespikeMaxRadius), side = 2 * radius + 1, n = side * side, centre = n / 2;
		const uint32_t rank = (uint32_t)(rng() % (n - 1));
		// exactly the values a window holds, each array a heap block of its own
		std::vector<double> SA(3 * n), QA(3 * n), SB(3 * n), QB(3 * n);
		std::vector<uint32_t> NA(n), NB(n);
		const bool one_count = rng() % 3 == 0; // a window inside one rect: every position at the same two counts
		const uint32_t ca = counts[1 + rng() % 8], cb = counts[1 + rng() % 8];
		for (uint32_t i = 0; i < n; i++) {
			NA[i] = one_count ? ca : counts[rng() % 9], NB[i] = one_count ? cb : counts[rng() % 9];
			const double m = means[rng() % (i == centre ? 13 : 12)], s2 = 0.01 * (double)(1 + rng() % 3);
			for (int c = 0; c < 3; c++) {
				const double na = (double)NA[i], nb = (double)NB[i];
				SA[3 * i + c] = m * na, SB[3 * i + c] = m * nb;
				QA[3 * i + c] = m * m * na + (NA[i] ? (na - 1.0) * s2 : 0.0), QB[3 * i + c] = m * m * nb + (NB[i] ? (nb - 1.0) * s2 : 0.0);
			}
			switch (rng() % 24) {
			case 0: SA[3 * i + rng() % 3] = nan; break;
			case 1: QB[3 * i + rng() % 3] = inf; break;
			case 2: SB[3 * i + rng() % 3] = -inf; break;
			case 3: SA[3 * i + 1] = SB[3 * i + 1] = 1.5e308; break; // finite halves, the sum overflows
			default: break;
			}
		}
		if (rng() % 2) { // a firefly: one sample in ONE half of the centre
			std::vector<double> &S = rng() % 2 ? SA : SB, &Q = (&S == &SA) ? QA : QB;
			for (int c = 0; c < 3; c++) S[3 * centre + c] += 500.0, Q[3 * centre + c] += 250000.0;
		}
		windows++;

		// ---- through the headers, the way the kernel drives them
		std::vector<double> Yw(n, nan), Vw(n, 0.0);
		for (uint32_t i = 0; i < n; i++) {
			double y, v;
			if (rmd::despike_dual_pixel(&SA[3 * i], &QA[3 * i], NA[i], &SB[3 * i], &QB[3 * i], NB[i], y, v)) Yw[i] = y, Vw[i] = v;
		}
		double got[12];
		for (int c = 0; c < 3; c++) got[c] = SA[3 * centre + c], got[3 + c] = QA[3 * centre + c], got[6 + c] = SB[3 * centre + c], got[9 + c] = QB[3 * centre + c];
		bool got_spike = false;
		const double k = (rng() % 4) ? 6.0 : 0.0, ratio = (rng() % 3) ? 2.0 : 1.0, floor = (rng() % 5) ? 0.0 : 0.25;
		const double yp = Yw[centre];
		int donor = -1;
		if (yp == yp && !rmd::despike_settled(rmd::despike_at_or_above(Yw.data(), side, radius, yp), rank, yp)) {
			donor = rmd::despike_donor(Yw.data(), side, radius, rank);
			if (donor >= 0 && rmd::despike_is_spike(yp, Yw[donor], Vw[donor], k, ratio, floor)) {
				got_spike = true;
				for (int c = 0; c < 3; c++) {
					got[c] = rmd::despike_dual_take(SA[3 * donor + c], NA[donor], NA[centre]), got[3 + c] = rmd::despike_dual_take(QA[3 * donor + c], NA[donor], NA[centre]);
					got[6 + c] = rmd::despike_dual_take(SB[3 * donor + c], NB[donor], NB[centre]), got[9 + c] = rmd::despike_dual_take(QB[3 * donor + c], NB[donor], NB[centre]);
				}
			}
		}

		// ---- the second plain reading
		double want[12];
		for (int c = 0; c < 3; c++) want[c] = SA[3 * centre + c], want[3 + c] = QA[3 * centre + c], want[6 + c] = SB[3 * centre + c], want[9 + c] = QB[3 * centre + c];
		bool want_spike = false;
		double Yp = 0, Vp = 0;
		if (plain_pixel(&SA[3 * centre], &QA[3 * centre], NA[centre], &SB[3 * centre], &QB[3 * centre], NB[centre], Yp, Vp)) {
			std::vector<Other> others;
			std::vector<double> Vo(n, 0.0);
			for (uint32_t i = 0; i < n; i++) {
				double y, v;
				if (i == centre) continue;
				if ((NA[i] == 0) != (NB[i] == 0)) empty_half_others++;
				if (!plain_pixel(&SA[3 * i], &QA[3 * i], NA[i], &SB[3 * i], &QB[3 * i], NB[i], y, v)) continue;
				others.push_back(Other{y, i}), Vo[i] = v;
			}
			std::stable_sort(others.begin(), others.end(), [](const Other &a, const Other &b) { return a.y > b.y; });
			if (rank < others.size()) {
				const uint32_t q = others[rank].i;
				volatile double rq = ratio * others[rank].y;
				volatile double e0 = Yp - rq;
				volatile double e = e0 - floor, k2 = k * k;
				volatile double ee = e * e, bound = k2 * Vo[q];
				if (e > 0.0 && ee > bound) {
					want_spike = true;
					const std::vector<double> *src[4] = {&SA, &QA, &SB, &QB};
					const uint32_t np[4] = {NA[centre], NA[centre], NB[centre], NB[centre]}, nq[4] = {NA[q], NA[q], NB[q], NB[q]};
					for (int h = 0; h < 4; h++)
						for (int c = 0; c < 3; c++) {
							const double d = (*src[h])[3 * q + c];
							if (np[h] == nq[h]) want[3 * h + c] = d;
							else {
								volatile double per = d / (double)nq[h];
								want[3 * h + c] = per * (double)np[h];
							}
						}
					const bool sa = NA[centre] != NA[q], sb = NB[centre] != NB[q];
					if (sa && sb) scaled_both++;
					else if (sa || sb) scaled_one_half++;
					else copied_both++;
				}
			} else without_donor++;
		} else {
			centre_invalid++;
			EXPECT(!(yp == yp), "window %" PRIu64 ": a centre the plain reading calls not valid has a Y", it);
		}
		EXPECT(got_spike == want_spike, "window %" PRIu64 ": radius %u rank %u, spike %d by the headers, %d by the plain reading", it, radius, rank, (int)got_spike, (int)want_spike);
		for (int j = 0; j < 12; j++) EXPECT(bits(got[j]) == bits(want[j]), "window %" PRIu64 ": output value %d, %a by the headers, %a by the plain reading", it, j, got[j], want[j]);
		if (want_spike) spikes++;
	}

	// ---- the edges
	{
		const double sa[3] = {8.0, 16.0, 4.0}, qa[3] = {9.0, 35.0, 3.0}, sb[3] = {8.0, 16.0, 4.0}, qb[3] = {8.5, 34.0, 2.5}, big[3] = {8.0, 1.5e308, 4.0}, bad[3] = {8.0, nan, 4.0};
		double s[3], q[3], Y = 0, V = 0, Y1 = 0, V1 = 0;
		rmd::despike_dual_merge(sa, qa, sb, qb, s, q);
		EXPECT(s[0] == 16.0 && s[1] == 32.0 && s[2] == 8.0 && q[0] == 17.5 && q[1] == 69.0 && q[2] == 5.5, "the merge");
		EXPECT(rmd::despike_dual_pixel(sa, qa, 8, sb, qb, 8, Y, V) && rmd::despike_pixel(s, q, 16, Y1, V1) && bits(Y) == bits(Y1) && bits(V) == bits(V1), "Y and V are rmd_despike's on the merged pixel");
		EXPECT(rmd::despike_dual_pixel(sa, qa, 1, sb, qb, 1, Y, V), "(1, 1) is valid: the merged count is 2");
		EXPECT(!rmd::despike_dual_pixel(sa, qa, 0, sb, qb, 8, Y, V) && !rmd::despike_dual_pixel(sa, qa, 8, sb, qb, 0, Y, V) && !rmd::despike_dual_pixel(sa, qa, 0, sb, qb, 0, Y, V),
		       "an empty half is not valid, whatever the merged count");
		EXPECT(!rmd::despike_dual_pixel(big, qa, 8, big, qb, 8, Y, V), "two finite halves whose sum overflows are not valid");
		EXPECT(!rmd::despike_dual_pixel(sa, qa, 8, bad, qb, 8, Y, V) && !rmd::despike_dual_pixel(sa, bad, 8, sb, qb, 8, Y, V), "a NaN in one half only is not valid");
		EXPECT(rmd::despike_dual_pixel(big, qa, 8, sa, qb, 8, Y, V), "a large finite half with a finite sum is valid");
		const double payload = [] {
			const uint64_t b = 0x7FF8000000000ABCull;
			double d;
			std::memcpy(&d, &b, sizeof d);
			return d;
		}();
		EXPECT(bits(rmd::despike_dual_take(payload, 8, 8)) == 0x7FF8000000000ABCull && bits(rmd::despike_dual_take(-0.0, 3, 3)) == bits(-0.0), "equal half counts: the donor's bits");
		EXPECT(rmd::despike_dual_take(10.0, 5, 16) == (10.0 / 5.0) * 16.0 && rmd::despike_dual_take(1.0, 3, 7) == rmd::despike_scaled(1.0, 3, 7), "other half counts: the scaled copy");
	}
	std::printf("despike dual rule %s: %" PRIu64 " windows, %" PRIu64 " with a centre that is not valid, %" PRIu64 " without a donor, %" PRIu64 " spikes, %" PRIu64
	            " copied in both halves, %" PRIu64 " scaled in one, %" PRIu64 " scaled in both, %" PRIu64 " others with one empty half\n",
	            failures ? "FAILED" : "ok", windows, centre_invalid, without_donor, spikes, copied_both, scaled_one_half, scaled_both, empty_half_others);
	return failures ? 1 : 0;
}
