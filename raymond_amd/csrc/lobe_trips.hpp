// The trip rule of the role-sorted spheres kernel (render_kernel.hpp: render_wave_sorted), as a function of the three numbers it depends on, so
// that it can be run on the CPU as well (tests/test_lobe_trip_policy.py drives it through random park / shade sequences).
//
// A wave keeps its parked hits in ONE array of `slots` entries used from both ends: the hits whose next bounce samples the diffuse lobe are
// pushed upward from entry 0 (n_d of them: entries 0 .. n_d - 1), the hits whose next bounce samples the GGX lobe downward from the last entry
// (n_g of them: entries slots - n_g .. slots - 1).  The two never overlap while n_d + n_g <= slots.
//   generation trip  while the item has pairs and n_d + n_g <= slots - 64: the 64 hits it may park fit, whatever their lobes;
//   shading trip     else, of the lobe that holds MORE hits (the diffuse one on a tie), popping its top min(n, 64).
// Progress: a shading trip runs only when no pair is left (then n_d + n_g > 0, or the loop has ended) or n_d + n_g > slots - 64, so the larger
// side holds at least one hit — more than (slots - 64) / 2 of them in the second case: 53 .. 64 lanes at 168 entries — and at least one path advances
// by a segment; a generation trip hands out 64 pairs.  No state selects a trip without a lane.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define RMD_LOBE_HD __host__ __device__ inline
#else
#define RMD_LOBE_HD inline
#endif

namespace rmd {

enum : uint32_t { kTripDone = 0, kTripGenerate = 1, kTripShadeDiffuse = 2, kTripShadeGgx = 3 };
struct LobeTrip {
	uint32_t kind;  // kTrip*
	uint32_t lanes; // shading: hits popped (1 .. 64); generation: 64 pairs handed out; done: 0
};
RMD_LOBE_HD LobeTrip lobe_trip_rule(uint32_t n_d, uint32_t n_g, bool items_left, uint32_t slots) {
	LobeTrip t;
	if (items_left && n_d + n_g + 64u <= slots) {
		t.kind = kTripGenerate, t.lanes = 64u;
	} else if (n_d + n_g == 0u) {
		t.kind = kTripDone, t.lanes = 0u; // (only without pairs left: slots >= 64)
	} else {
		const bool diffuse = n_d >= n_g;
		const uint32_t n = diffuse ? n_d : n_g;
		t.kind = diffuse ? kTripShadeDiffuse : kTripShadeGgx, t.lanes = n < 64u ? n : 64u;
	}
	return t;
}
// The trip loop's bound (render_kernel.hpp: report_fault): every trip hands out 64 pairs or advances at least one path by a segment, so an item of
// `pool_items` pairs whose paths have at most per_pair - 4 segments each ends within this many trips even if every trip served ONE lane.
RMD_LOBE_HD unsigned long long lobe_trip_bound(uint32_t pool_items, uint32_t per_pair) { return (unsigned long long)pool_items * per_pair + 64ull; }
// first entry a shading trip of `lanes` hits pops (lane i: entry first + i), and the entry a lane of rank `rank` among a trip's parking lanes of one lobe pushes to
RMD_LOBE_HD uint32_t lobe_pop_first(bool diffuse, uint32_t n_d, uint32_t n_g, uint32_t lanes, uint32_t slots) { return diffuse ? n_d - lanes : slots - n_g; }
RMD_LOBE_HD uint32_t lobe_push_entry(bool diffuse, uint32_t n_d, uint32_t n_g, uint32_t rank, uint32_t slots) { return diffuse ? n_d + rank : slots - 1u - n_g - rank; }

} // namespace rmd
