// The work list of a split launch of the role-sorted spheres kernel (render_kernel.hpp: render_wave_sorted), as functions of plain numbers that
// the kernel and the host share (tests/test_work_list.py walks them on the CPU through rmd_probe_work_plan / rmd_probe_work_items).
//
// A work item is (wave tile, sample range).  The list has two parts, handed out in this order by the launch's counter:
//   whole items   items 0 .. n_whole - 1: wave tile i with ALL samples of the pass — part 0 of 1.  One wave computes, stores and adds the tile's
//                 samples: no other wave has to see them (render_kernel.hpp: finish_sample_range), the wave drains its hit stacks once and derives
//                 the tile's candidate set once;
//   tail items    the remaining n_tiles - n_whole wave tiles, k_tail items each, a tile's parts next to each other and in sample order: part p holds
//                 samples p * ceil(sample_count / k_tail) onwards (parts past the last sample are empty and still counted by tile_done).
// Items exist to level the END of the launch over the wave slots, so only the end is fine-grained.  n_whole = 0 is the uniform split every other
// kernel runs and a forced RMD_TUNE_SAMPLE_SPLIT keeps: item = tile * k + part.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define RMD_WORK_HD __host__ __device__ inline
#else
#define RMD_WORK_HD inline
#endif

namespace rmd {

struct WorkItem {
	uint32_t tile;  // the wave tile; n_tiles for an item past the end of the list (count = 0 then)
	uint32_t first; // first sample of the pass (0 .. sample_count) ...
	uint32_t count; // ... and how many
	uint32_t parts; // items this tile's samples are spread over: what tile_done counts to (1 for a whole item)
	uint32_t whole; // 1: the item holds all of its tile's samples and its wave alone adds them
};
// items of the list (api.cpp keeps it below 2^31: kWorkCounterPoison)
RMD_WORK_HD uint32_t work_list_items(uint32_t n_tiles, uint32_t n_whole, uint32_t k_tail) { return n_whole + (n_tiles - n_whole) * k_tail; }
// item -> (tile, first sample, sample count, parts of this tile); n_whole <= n_tiles, k_tail >= 1
RMD_WORK_HD WorkItem work_list_item(uint32_t item, uint32_t n_tiles, uint32_t n_whole, uint32_t k_tail, uint32_t sample_count) {
	WorkItem w;
	if (item < n_whole) {
		w.tile = item, w.first = 0u, w.count = sample_count, w.parts = 1u, w.whole = 1u;
	} else {
		const uint32_t t = item - n_whole, q = t / k_tail, part = t - q * k_tail;
		const uint32_t per_part = (sample_count + k_tail - 1u) / k_tail;
		const uint32_t s_lo = part * per_part < sample_count ? part * per_part : sample_count;
		const uint32_t s_hi = s_lo + per_part < sample_count ? s_lo + per_part : sample_count;
		w.tile = n_whole + q, w.first = s_lo, w.count = s_hi - s_lo, w.parts = k_tail, w.whole = 0u;
	}
	if (w.tile >= n_tiles) w.tile = n_tiles, w.count = 0u; // (a launch of one wave per item may hold a few waves more than items)
	return w;
}

// The plan (api.cpp: plan_work_list makes it): n_whole + n_tail is the tile count
struct WorkPlan {
	uint32_t n_whole, n_tail, k_tail;
};
// A whole item numbers its (pixel, sample) pairs 0 .. sample_count * 64 - 1 in the 32-bit field of a parked hit (render_kernel.hpp: HitStack::item)
// and bounds its trips by lobe_trip_bound(pairs, ..): whole items are planned only for passes of at most 2^20 samples — pairs below 2^26, with
// six bits to spare.  A longer pass stays uniformly split.
constexpr uint32_t kWholeMaxSamples = 1u << 20;
// tail tiles per wave slot, in halves (c = 2.5: api.cpp, plan_work_list, has the measurements), and the parts a tail tile is cut into where the samples
// allow (at least kTailMinSamples each)
constexpr uint32_t kTailTilesPerSlotX2 = 5u;
constexpr uint32_t kTailParts = 4u;
constexpr uint32_t kTailMinSamples = 64u;

} // namespace rmd
