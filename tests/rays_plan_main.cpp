// rays_plan.hpp (the launch plan of rmd_intersect_rays) on the CPU, as a program of its own: built with -fsanitize=address,undefined by
// tests/test_rays_host.py and run there.  For every n of the sweep, CU count and waves per workgroup it walks the batch loop exactly as the kernel
// does — wave u takes u, u + total_waves, ... below `batches` — and checks that the batches taken are [0, ceil(n / 64)) exactly once each, that
// every wave's trip count is rays_plan_trips, that no ray index passes 2^31, and the plan's own sums.
//   rays_plan_main            prints "rays plan ok: <plans> plans, <batches> batches walked, <looping> with waves that loop, largest n <n>"
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "rays_plan.hpp"

static unsigned long long n_plans = 0, n_walked = 0, n_looping = 0, largest = 0;

static void fail(const char *what, unsigned long long n, unsigned cus, unsigned wpw) {
	std::fprintf(stderr, "rays plan: %s at n = %llu, %u CUs, %u waves per workgroup\n", what, n, cus, wpw);
	std::exit(1);
}

static void check(unsigned long long n, unsigned cus, unsigned wpw, std::vector<unsigned char> &seen) {
	const rmd::RaysPlan p = rmd::rays_plan(n, cus, wpw);
	const unsigned long long batches = (n + 63u) / 64u;
	if (p.batches != batches || p.waves_per_wg != wpw) fail("batches or waves per workgroup", n, cus, wpw);
	if (n == 0) {
		if (p.workgroups != 0 || p.total_waves != 0) fail("a launch for no rays", n, cus, wpw);
		n_plans++;
		return;
	}
	const unsigned long long cap = (unsigned long long)cus * rmd::kRaysSlotsPerCu * rmd::kRaysFill;
	if (p.workgroups == 0 || p.total_waves != (unsigned long long)p.workgroups * wpw) fail("total waves", n, cus, wpw);
	if (p.total_waves >= (batches < cap ? batches : cap) + wpw) fail("more than one workgroup's spare waves", n, cus, wpw);
	if (p.total_waves < (batches < cap ? batches : cap)) fail("fewer waves than batches below the cap", n, cus, wpw);
	seen.assign((size_t)batches, 0);
	unsigned long long taken = 0;
	bool loops = false;
	for (uint32_t u = 0; u < p.total_waves; u++) {
		uint32_t trips = 0;
		for (uint32_t b = u; b < p.batches; b += p.total_waves) { // the kernel's loop
			if ((unsigned long long)b * 64u + 63u >= (1ull << 31)) fail("a ray index past 2^31", n, cus, wpw);
			if (seen[b]++) fail("a batch taken twice", n, cus, wpw);
			trips++;
		}
		if (trips != rmd::rays_plan_trips(p, u)) fail("rays_plan_trips", n, cus, wpw);
		loops = loops || trips > 1;
		taken += trips;
	}
	if (taken != batches) fail("a batch not taken", n, cus, wpw);
	for (size_t b = 0; b < seen.size(); b++)
		if (seen[b] != 1) fail("a batch not taken exactly once", n, cus, wpw);
	if (rmd::rays_plan_trips(p, p.total_waves) != 0 && p.total_waves >= p.batches) fail("trips of a wave past the launch", n, cus, wpw);
	n_plans++, n_walked += batches, n_looping += loops;
	if (n > largest) largest = n;
}

int main() {
	static_assert(RMD_RAYS_MAX_RAYS == (1ull << 30), "the sweep's upper end");
	const unsigned cu_counts[3] = {1, 8, 256};
	std::vector<unsigned char> seen;
	std::set<unsigned long long> ns = {0, 1, 63, 64, 65};
	for (unsigned long long n = 0; n <= 1025; n++) ns.insert(n);
	for (unsigned cus : cu_counts)
		for (unsigned wpw = 1; wpw <= 4; wpw++) {
			// the products and neighbours of the plan's wave counts: where the cap begins to hold, and whole multiples of the launch's waves
			const unsigned long long cap = (unsigned long long)cus * rmd::kRaysSlotsPerCu * rmd::kRaysFill;
			const unsigned long long waves = (cap + wpw - 1) / wpw * wpw;
			for (unsigned long long w : {cap, waves})
				for (unsigned long long k : {1ull, 2ull, 3ull, 7ull})
					for (long long d : {-65ll, -64ll, -63ll, -1ll, 0ll, 1ll, 63ll, 64ll, 65ll}) ns.insert(w * k * 64ull + (unsigned long long)d);
		}
	for (unsigned long long n : ns)
		for (unsigned cus : cu_counts)
			for (unsigned wpw = 1; wpw <= 4; wpw++) check(n, cus, wpw, seen);
	for (unsigned long long n : {(1ull << 30) - 65, (1ull << 30) - 64, (1ull << 30) - 63, (1ull << 30) - 1, 1ull << 30})
		for (unsigned pair : {0x11u, 0x84u, 0x1001u, 0x1004u}) check(n, pair >> 4, pair & 15u, seen); // 1 CU x 1 wave, 8 x 4, 256 x 1, 256 x 4
	// a CU count or a wave count of 0 counts as 1
	const rmd::RaysPlan a = rmd::rays_plan(1000, 0, 0), b = rmd::rays_plan(1000, 1, 1);
	if (a.batches != b.batches || a.workgroups != b.workgroups || a.total_waves != b.total_waves || a.waves_per_wg != 1) fail("zero counts", 1000, 0, 0);
	std::printf("rays plan ok: %llu plans, %llu batches walked, %llu with waves that loop, largest n %llu\n", n_plans, n_walked, n_looping, largest);
	return 0;
}
