// Drives the trip rule of the role-sorted spheres kernel (raymond_amd/csrc/lobe_trips.hpp) through seeded random park / shade sequences on the CPU
// (tests/test_lobe_trip_policy.py builds this with -fsanitize=address,undefined and runs it).
//   usage: lobe_trip_policy SLOTS TRIP_BOUND_PER_PAIR MAX_SEGMENTS FIRST_SEQUENCE SEQUENCES
// A sequence is one work item: 1 .. 200 generation trips of 64 pairs (every size with every share; nine sequences in ten are items of 1 .. 16 trips,
// where the drain rule and stacks that never fill decide); a primary hit parks with a probability drawn per sequence, a shaded hit parks
// again with another, a path has at most MAX_SEGMENTS segments, a parked hit's lobe is GGX with the sequence's share (0, 0.1, 0.5, 0.9, 1 in turn).
// The array's entries are tracked one by one (free / diffuse / GGX, and the depth of the path parked there), with the header's own index functions.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "lobe_trips.hpp"

static uint64_t rng_state;
static double uniform() { // splitmix64 -> [0, 1)
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	z ^= z >> 31;
	return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
#define CHECK(c, ...)                                    \
	do {                                                 \
		if (!(c)) {                                      \
			fprintf(stderr, "FAILED: %s: ", #c);         \
			fprintf(stderr, __VA_ARGS__);                \
			fprintf(stderr, "\n");                       \
			exit(1);                                     \
		}                                                \
	} while (0)

int main(int argc, char **argv) {
	if (argc != 6) return 2;
	const uint32_t slots = (uint32_t)atoi(argv[1]), per_pair = (uint32_t)atoi(argv[2]), max_segments = (uint32_t)atoi(argv[3]);
	const long first_sequence = atol(argv[4]), sequences = atol(argv[5]);
	const double shares[5] = {0.0, 0.1, 0.5, 0.9, 1.0};
	unsigned long long trips_total = 0, shade_trips[2] = {0, 0}, shade_lanes[2] = {0, 0}, worst_fill = 0;
	for (long seq = first_sequence; seq < first_sequence + sequences; seq++) {
		rng_state = 0x5EED0001ull + (uint64_t)seq * 0x1000003ull;
		const double share = shares[seq % 5];
		const long j = seq / 5;
		const uint32_t gen_trips = j % 10 == 0 ? 1u + (uint32_t)((j / 10) % 200) : 1u + (uint32_t)(j % 16);
		const double p_primary = uniform(), p_again = seq % 7 == 0 ? 1.0 : uniform(); // (every seventh: every path runs to the bounce limit)
		const uint32_t pool_items = gen_trips * 64u;
		std::vector<uint8_t> owner(slots, 0); // 0 free, 1 diffuse, 2 GGX
		std::vector<uint8_t> segs(slots, 0);  // segments the path parked there has run
		uint32_t n_d = 0, n_g = 0, next_item = 0;
		unsigned long long trips = 0;
		const unsigned long long bound = rmd::lobe_trip_bound(pool_items, per_pair);
		for (;;) {
			const rmd::LobeTrip trip = rmd::lobe_trip_rule(n_d, n_g, next_item < pool_items, slots);
			if (trip.kind == rmd::kTripDone) break;
			trips++;
			CHECK(trips <= bound, "sequence %ld: %llu trips, bound %llu", seq, trips, bound);
			CHECK(trip.lanes >= 1u && trip.lanes <= 64u, "sequence %ld: a trip of %u lanes", seq, trip.lanes);
			uint8_t parked_segs[64];
			uint32_t n_run = 0; // paths this trip runs a segment of, and how many segments each has behind it afterwards
			if (trip.kind == rmd::kTripGenerate) {
				CHECK(next_item < pool_items, "sequence %ld: a generation trip without pairs", seq);
				CHECK(n_d + n_g + 64u <= slots, "sequence %ld: a generation trip with %u + %u hits waiting", seq, n_d, n_g);
				next_item += 64u;
				for (uint32_t i = 0; i < 64u; i++)
					if (uniform() < p_primary && 1u < max_segments) parked_segs[n_run++] = 1;
			} else {
				const bool diffuse = trip.kind == rmd::kTripShadeDiffuse;
				CHECK(trip.kind == rmd::kTripShadeGgx || diffuse, "sequence %ld: trip kind %u", seq, trip.kind);
				CHECK(trip.lanes <= (diffuse ? n_d : n_g), "sequence %ld: %u lanes of %u hits", seq, trip.lanes, diffuse ? n_d : n_g);
				CHECK((diffuse ? n_d : n_g) >= (diffuse ? n_g : n_d), "sequence %ld: the emptier stack is shaded", seq);
				const uint32_t first = rmd::lobe_pop_first(diffuse, n_d, n_g, trip.lanes, slots);
				for (uint32_t i = 0; i < trip.lanes; i++) {
					const uint32_t e = first + i;
					CHECK(e < slots && owner[e] == (diffuse ? 1 : 2), "sequence %ld: entry %u popped as %s holds %u", seq, e, diffuse ? "diffuse" : "GGX", e < slots ? owner[e] : 99u);
					owner[e] = 0;
					const uint8_t s = (uint8_t)(segs[e] + 1u); // the bounce ray's segment
					if (s < max_segments && uniform() < p_again) parked_segs[n_run++] = s;
				}
				if (diffuse) n_d -= trip.lanes;
				else n_g -= trip.lanes;
				shade_trips[diffuse ? 0 : 1]++, shade_lanes[diffuse ? 0 : 1] += trip.lanes;
			}
			// the push: each lobe's lanes by their rank among their own kind
			uint32_t rank[2] = {0, 0};
			for (uint32_t i = 0; i < n_run; i++) {
				const bool diffuse = !(uniform() < share);
				const uint32_t e = rmd::lobe_push_entry(diffuse, n_d, n_g, rank[diffuse ? 0 : 1]++, slots);
				CHECK(e < slots && owner[e] == 0, "sequence %ld: entry %u pushed to holds %u (n_d %u, n_g %u)", seq, e, e < slots ? owner[e] : 99u, n_d, n_g);
				owner[e] = diffuse ? 1 : 2, segs[e] = parked_segs[i];
			}
			n_d += rank[0], n_g += rank[1];
			CHECK(n_d + n_g <= slots, "sequence %ld: %u + %u hits in %u entries", seq, n_d, n_g, slots);
			if (n_d + n_g > worst_fill) worst_fill = n_d + n_g;
			// the two stacks are what the counters say: entries 0 .. n_d - 1 diffuse, slots - n_g .. slots - 1 GGX, free between
			for (uint32_t e = 0; e < slots && (trips & 7u) == 0u; e++) { // (every eighth trip: a push or pop onto a wrong entry stops the run at once, above)
				const uint8_t want = e < n_d ? 1 : e >= slots - n_g ? 2 : 0;
				CHECK(owner[e] == want, "sequence %ld: entry %u holds %u, the counters say %u", seq, e, owner[e], want);
			}
		}
		CHECK(next_item >= pool_items && n_d == 0 && n_g == 0, "sequence %ld ended with work left", seq);
		trips_total += trips;
	}
	printf("lobe trip policy ok: %ld sequences, %llu trips, fullest %llu of %u entries, diffuse trips %llu (%.1f lanes), GGX trips %llu (%.1f lanes)\n", sequences, trips_total, worst_fill,
	       slots, shade_trips[0], shade_trips[0] ? (double)shade_lanes[0] / shade_trips[0] : 0.0, shade_trips[1], shade_trips[1] ? (double)shade_lanes[1] / shade_trips[1] : 0.0);
	return 0;
}
