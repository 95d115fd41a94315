// The host arithmetic of rmd_resolve_tonemap_tiles (api_frame.cpp; the kernel is resolve_tiles.hip): where a rect's pixels lie in the packed output, the
// table that gives every workgroup its pixels, and the way back from a flagged packed pixel to its rect and frame position.  Needs only <stdint.h>
// and the standard library — `Rect` is any struct with left, top, width, height (rmd_tile_rect) — so that it can be run on the CPU by itself
// (tests/resolve_tiles_table_main.cpp drives it through random rect lists).
//
// Packed order: rect j's pixels row-major, one rect after the other (rmd_framebuffer_download_tiles's layout).  first[j] = packed pixels in front of
// rect j, first[n_rects] = all of them.  A rect without pixels has first[j] == first[j + 1].
//
// The packed pixels are cut into CHUNKS of kResolveRun = 1024 at multiples of 1024, and a chunk at every rect boundary inside it: each piece is one
// ResolveRun, the work of one workgroup.  So a run lies in one rect, never crosses a multiple of 1024 — its lanes' groups of kResolveGroup = 4 packed
// pixels, 12 bytes at a multiple of 12, number at most 256 — and the runs in table order cover 0 .. first[n_rects] - 1 once each without a gap.  One
// large rect gives a run per 1024 pixels, 32 x 32 tiles one run each (two where ragged tiles in front have shifted them off the multiples): the number
// of workgroups follows the pixels, plus at most one per rect.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace rmd {

constexpr uint32_t kResolveGroup = 4u;  // packed pixels per lane: 12 bytes, three whole dwords of the packed output
constexpr uint32_t kResolveRun = 1024u; // packed pixels per workgroup at most: 256 lanes
static_assert(kResolveRun == 256u * kResolveGroup, "a workgroup of 256 lanes covers one chunk");

struct ResolveRun {
	uint32_t rect;        // index into the caller's rects
	uint32_t left, top;   // the rect's corner in the frame
	uint32_t width;       // the rect's width (> 0: a rect without pixels has no run)
	uint32_t local;       // the run's first pixel, counted row-major inside the rect
	uint32_t start;       // ... and in the packed output
	uint32_t n;           // pixels of the run, 1 .. kResolveRun
	uint32_t samples;     // the rect's sample count
};
static_assert(sizeof(ResolveRun) == 32, "the kernel reads the table as eight words per run");

// first: n_rects + 1 entries.  Returns false when a rect reaches outside the width x height frame (first is then unspecified).
template <class Rect>
bool resolve_first_pixels(const Rect *rects, uint32_t n_rects, uint32_t width, uint32_t height, std::vector<uint64_t> &first) {
	first.resize((size_t)n_rects + 1);
	uint64_t at = 0;
	for (uint32_t j = 0; j < n_rects; j++) {
		const Rect &r = rects[j];
		if ((uint64_t)r.left + r.width > width || (uint64_t)r.top + r.height > height) return false;
		first[j] = at;
		at += (uint64_t)r.width * r.height;
	}
	first[n_rects] = at;
	return true;
}

// The workgroup table.  first[n_rects] must fit 32 bits (the caller refuses more).
template <class Rect>
std::vector<ResolveRun> resolve_runs(const Rect *rects, const uint32_t *samples, uint32_t n_rects, const std::vector<uint64_t> &first) {
	std::vector<ResolveRun> runs;
	runs.reserve((size_t)(first[n_rects] / kResolveRun) + n_rects + 1);
	for (uint32_t j = 0; j < n_rects; j++) {
		const uint64_t end = first[j + 1];
		for (uint64_t at = first[j]; at < end;) {
			const uint64_t stop = std::min(end, (at / kResolveRun + 1) * kResolveRun);
			runs.push_back(ResolveRun{j, rects[j].left, rects[j].top, rects[j].width, (uint32_t)(at - first[j]), (uint32_t)at, (uint32_t)(stop - at), samples[j]});
			at = stop;
		}
	}
	return runs;
}

struct ResolvePixel {
	uint32_t rect; // the rect that holds packed pixel `packed`
	uint32_t x, y; // ... and the pixel's position in the frame
};
// packed < first[n_rects]: the last rect whose first pixel is at or before it (rects without pixels, which share their successor's, are passed over)
template <class Rect>
ResolvePixel resolve_locate(const Rect *rects, uint32_t n_rects, const std::vector<uint64_t> &first, uint64_t packed) {
	const uint32_t j = (uint32_t)(std::upper_bound(first.begin(), first.begin() + n_rects, packed) - first.begin()) - 1u;
	const uint64_t local = packed - first[j];
	return ResolvePixel{j, rects[j].left + (uint32_t)(local % rects[j].width), rects[j].top + (uint32_t)(local / rects[j].width)};
}

} // namespace rmd
