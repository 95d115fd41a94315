// The pure host arithmetic of the denoise entry points (api_denoise.cpp): the layout of their device scratch and the block tables of the region forms.
// No HIP call and no context — this header needs include/raymond_hip.h alone —, so all of it is checked off the GPU (rmd_probe_denoise_scratch,
// tests/test_denoise_scratch_layout.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/raymond_hip.h"

namespace rmd {

// One workgroup's share of a region call: its tile's origin, and the far corner (exclusive) of the rect the tile was cut from
struct alignas(16) DualBlock {
	uint32_t x0, y0, x_end, y_end;
};

// ---------------------------------------------------------------- the scratch block
// the filters that carve a block (include/raymond_hip_probe.h: RMD_PROBE_SCRATCH_*) ...
enum ScratchForm {
	kScratchSingle = 0,        // rmd_denoise, rmd_denoise_guided
	kScratchAtrous,            // rmd_denoise_atrous
	kScratchDual,              // rmd_denoise_dual[_guided][_region]
	kScratchAtrousDual,        // rmd_denoise_atrous_dual
	kScratchAtrousDualRegion,  // rmd_denoise_atrous_dual_region
	kScratchDualSelect,        // rmd_denoise_dual_select
	kScratchTileError,         // rmd_tile_error_dual
	kScratchForms
};
// ... and the parts a block may hold, as launch.hpp names and sizes them
enum ScratchPart {
	kPartPlanes = 0,  // doubles: cv (12 * W*H), the dual planes (12 * W*H) or the a-trous dual state (24 * W*H)
	kPartFb,          // f_b, 3 * W*H doubles
	kPartCand,        // cand_img, 7 * W*H doubles per candidate
	kPartGain,        // gain, 2 * W*H doubles
	kPartFeatPlanes,  // feat_planes, 14 * W*H doubles
	kPartCountImg,    // n_img, W*H uint32 (dual forms: 2 * W*H)
	kPartWinImg,      // win_img, W*H uint32
	kPartFeatCountImg, // n_f_img, W*H uint32
	kPartTable,       // DualBlock entries
	kPartRects,       // the frame's rects
	kPartCountsA,     // their counts, n_rects uint32 each
	kPartCountsB,
	kPartCountsF,
	kPartTileErrors,  // rmd_tile_error_dual's result, n_rects doubles
	kPartSlopePlanes, // slope_planes, 7 * W*H doubles (the _slope calls with a slope > 0; the non-local-means blocks hold it right behind feat_planes, the a-trous blocks last)
	kScratchParts
};
struct ScratchLayout {
	bool used[kScratchParts] = {}; // (a part that is not used has no pointer: the launchers tell the guided and the region calls by them)
	size_t offset[kScratchParts] = {}, bytes[kScratchParts] = {};
	size_t total = 0;
};
// The block of one call.  Every part starts on a 16-byte boundary.  `guided`: the call has features (rmd_denoise_dual_select: a guided candidate);
// n_table: the entries of the region forms' block tables (rmd_denoise_dual[_guided]_region, rmd_denoise_atrous_dual_region), 0 for a whole-frame call;
// the other forms take no table and ignore it; `sloped`: a guided non-local-means _slope call (single, dual, dual_select) some slope of which is > 0;
// `atrous_sloped`: a guided a-trous _slope call (atrous, atrous_dual, atrous_dual_region) whose slope is > 0 — without them every block is what it was before the
// slope existed.  The non-local-means blocks hold the slope planes right behind the feature planes, the a-trous blocks behind everything else: every other
// part of theirs keeps its offset.  (Two flags: `sloped` is pinned to change nothing on the a-trous forms.)
inline ScratchLayout denoise_scratch_layout(ScratchForm form, uint32_t W, uint32_t H, uint32_t n_rects, bool guided, uint32_t n_cands, size_t n_table,
                                            bool sloped = false, bool atrous_sloped = false) {
	ScratchLayout L;
	const size_t N = (size_t)W * H, f64 = sizeof(double), u32 = sizeof(uint32_t);
	auto part = [&](ScratchPart p, size_t elem_bytes, size_t count, bool wanted = true) {
		if (!wanted) return;
		L.used[p] = true, L.offset[p] = L.total, L.bytes[p] = elem_bytes * count;
		L.total += (L.bytes[p] + 15u) & ~(size_t)15u;
	};
	const bool dual = form == kScratchDual || form == kScratchAtrousDual || form == kScratchAtrousDualRegion || form == kScratchDualSelect;
	switch (form) {
	case kScratchSingle: break;
	case kScratchAtrous: part(kPartPlanes, f64, 12u * N); break;
	case kScratchDual: part(kPartPlanes, f64, 12u * N), part(kPartFb, f64, 3u * N); break;
	case kScratchAtrousDual:
	case kScratchAtrousDualRegion: part(kPartPlanes, f64, 24u * N); break;
	case kScratchDualSelect: part(kPartPlanes, f64, 12u * N), part(kPartCand, f64, 7u * N * n_cands), part(kPartGain, f64, 2u * N), part(kPartWinImg, u32, N); break;
	default: break;
	}
	if (form != kScratchTileError) {
		part(kPartCountImg, u32, dual ? 2u * N : N);
		part(kPartFeatPlanes, f64, 2u * RMD_FEATURE_CHANNELS * N, guided);
		part(kPartSlopePlanes, f64, RMD_FEATURE_CHANNELS * N, guided && sloped && (form == kScratchSingle || form == kScratchDual || form == kScratchDualSelect));
		part(kPartFeatCountImg, u32, N, guided && dual);
		part(kPartTable, sizeof(DualBlock), n_table, n_table != 0u && (form == kScratchDual || form == kScratchAtrousDualRegion)); // (the region launchers alone)
	}
	part(kPartRects, sizeof(rmd_tile_rect), n_rects);
	part(kPartCountsA, u32, n_rects, form != kScratchTileError);
	part(kPartCountsB, u32, n_rects, dual);
	part(kPartCountsF, u32, n_rects, guided && dual);
	part(kPartTileErrors, f64, n_rects, form == kScratchTileError);
	part(kPartSlopePlanes, f64, RMD_FEATURE_CHANNELS * N, guided && atrous_sloped && (form == kScratchAtrous || form == kScratchAtrousDual || form == kScratchAtrousDualRegion));
	return L;
}

// rmd_despike's block, in the parts' existing names: kPartCountImg the per-pixel counts, kPartWinImg the per-pixel rect index (W*H uint32 each),
// kPartRects and kPartCountsA the rects and their counts, kPartTileErrors the per-rect spike counters (n_rects uint32).  Not one of the forms above: no
// filter's block changes, and the probe of those layouts does not list it
inline ScratchLayout despike_scratch_layout(uint32_t W, uint32_t H, uint32_t n_rects) {
	ScratchLayout L;
	const size_t N = (size_t)W * H, u32 = sizeof(uint32_t);
	auto part = [&](ScratchPart p, size_t elem_bytes, size_t count) {
		L.used[p] = true, L.offset[p] = L.total, L.bytes[p] = elem_bytes * count;
		L.total += (L.bytes[p] + 15u) & ~(size_t)15u;
	};
	part(kPartCountImg, u32, N), part(kPartWinImg, u32, N);
	part(kPartRects, sizeof(rmd_tile_rect), n_rects), part(kPartCountsA, u32, n_rects), part(kPartTileErrors, u32, n_rects);
	return L;
}

// rmd_despike_dual's block: rmd_despike's with both halves' count images in kPartCountImg (2 * W*H uint32, half A's first) and kPartCountsB beside
// kPartCountsA
inline ScratchLayout despike_dual_scratch_layout(uint32_t W, uint32_t H, uint32_t n_rects) {
	ScratchLayout L;
	const size_t N = (size_t)W * H, u32 = sizeof(uint32_t);
	auto part = [&](ScratchPart p, size_t elem_bytes, size_t count) {
		L.used[p] = true, L.offset[p] = L.total, L.bytes[p] = elem_bytes * count;
		L.total += (L.bytes[p] + 15u) & ~(size_t)15u;
	};
	part(kPartCountImg, u32, 2u * N), part(kPartWinImg, u32, N);
	part(kPartRects, sizeof(rmd_tile_rect), n_rects), part(kPartCountsA, u32, n_rects), part(kPartCountsB, u32, n_rects), part(kPartTileErrors, u32, n_rects);
	return L;
}

// The block of rmd_tile_luma_error (n_table 0) and rmd_tile_weighted_error (n_table RMD_LUMA_WEIGHTS), in the parts' existing names: kPartRects and
// kPartCountsA the rects and their counts, kPartTable the call's table of n_table doubles, kPartTileErrors the per-rect results of result_bytes each.  All
// but the results is what the call uploads, in one copy: those parts lie at the block's start in this order, each padded to 16 bytes; `upload_bytes` is
// where the results begin.  Like rmd_despike's it is not one of the forms above
inline ScratchLayout tile_measure_scratch_layout(uint32_t n_rects, size_t result_bytes, size_t n_table, size_t *upload_bytes) {
	ScratchLayout L;
	auto part = [&](ScratchPart p, size_t elem_bytes, size_t count) {
		L.used[p] = true, L.offset[p] = L.total, L.bytes[p] = elem_bytes * count;
		L.total += (L.bytes[p] + 15u) & ~(size_t)15u;
	};
	part(kPartRects, sizeof(rmd_tile_rect), n_rects), part(kPartCountsA, sizeof(uint32_t), n_rects);
	if (n_table != 0u) part(kPartTable, sizeof(double), n_table);
	*upload_bytes = L.total;
	part(kPartTileErrors, result_bytes, n_rects);
	return L;
}

// The block of rmd_tile_weighted_error_dual: kPartRects the rects and kPartTable the RMD_LUMA_WEIGHTS weights, uploaded in one copy of `upload_bytes` from
// the block's start, then kPartTileErrors the per-rect results.  The measure reads no counts, so the block has none
inline ScratchLayout tile_weighted_dual_scratch_layout(uint32_t n_rects, size_t result_bytes, size_t n_table, size_t *upload_bytes) {
	ScratchLayout L;
	auto part = [&](ScratchPart p, size_t elem_bytes, size_t count) {
		L.used[p] = true, L.offset[p] = L.total, L.bytes[p] = elem_bytes * count;
		L.total += (L.bytes[p] + 15u) & ~(size_t)15u;
	};
	part(kPartRects, sizeof(rmd_tile_rect), n_rects), part(kPartTable, sizeof(double), n_table);
	*upload_bytes = L.total;
	part(kPartTileErrors, result_bytes, n_rects);
	return L;
}

// ---------------------------------------------------------------- the block tables of the region forms
// rmd_denoise_dual_region: each region rect cut into tiles of the kernel's own shape (tw x th) from the rect's corner, row by row
inline std::vector<DualBlock> dual_region_table(const rmd_tile_rect *region, uint32_t n_region, uint32_t tw, uint32_t th) {
	std::vector<DualBlock> table;
	for (uint32_t i = 0; i < n_region; i++) {
		const rmd_tile_rect &r = region[i];
		for (uint32_t y = 0; y < r.height; y += th)
			for (uint32_t x = 0; x < r.width; x += tw) table.push_back(DualBlock{r.left + x, r.top + y, r.left + r.width, r.top + r.height});
	}
	return table;
}

// rmd_denoise_atrous_dual_region: the block tables, one after another in `table` — [0] the prologue's, [1 + l] level l's; table t is entries first[t] .. +
// count[t].  too_large: 0, or which of the two limits of 2^31 - 1 workgroups was passed (the tables are then not complete)
struct AtrousRegionTables {
	std::vector<DualBlock> table;
	std::vector<uint32_t> first, count;
	enum { kFits = 0, kFrameTooLarge, kRegionTooLarge } too_large = kFits;
};
// The needed sets: the last level's output is needed on the region; level l's on R_l = R_{l+1}
// dilated by 2 * 2^(l+1) pixels each way — a level-(l+1) tap reaches two steps of 2^(l+1) — clipped to the frame; the prologue's planes on R_0 dilated by 2.
// Dilating a union of rects is dilating each, and clipping after every step is clipping once, so R_l is the region's rects each grown by
// 2 * (2^levels - 2^(l+1)) and the prologue's set by 2 * (2^levels - 1).
// BW x BH: the kernels' workgroup (denoise_atrous_dual.hip: kAtrousDualBlockW x kAtrousDualBlockH) — constants, so that the divisions by them are shifts
template <uint32_t BW, uint32_t BH>
AtrousRegionTables atrous_region_tables(const rmd_tile_rect *region, uint32_t n_region, uint32_t width, uint32_t height, uint32_t levels) {
	constexpr uint32_t bw = BW, bh = BH;
	AtrousRegionTables T;
	// The region as the host cuts it: rects of one top and height that abut left to right are joined (they are disjoint, so the pixels are the same) — a
	// row of live 32 x 32 tiles then fills the 64-wide blocks of the last level instead of half of each.  Rects without pixels are dropped.
	std::vector<rmd_tile_rect> joined;
	{
		std::vector<uint32_t> order;
		for (uint32_t i = 0; i < n_region; i++)
			if (region[i].width != 0 && region[i].height != 0) order.push_back(i);
		std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
			const rmd_tile_rect &p = region[a], &q = region[b];
			return p.top != q.top ? p.top < q.top : p.height != q.height ? p.height < q.height : p.left < q.left;
		});
		for (uint32_t i : order) {
			const rmd_tile_rect &r = region[i];
			if (!joined.empty() && joined.back().top == r.top && joined.back().height == r.height && joined.back().left + joined.back().width == r.left) joined.back().width += r.width;
			else joined.push_back(r);
		}
	}
	region = joined.data(), n_region = (uint32_t)joined.size();
	std::vector<DualBlock> &table = T.table;
	T.first.resize(levels + 1u), T.count.resize(levels + 1u);
	const uint64_t tiles_x = ((uint64_t)width + bw - 1u) / bw, tiles_y = ((uint64_t)height + bh - 1u) / bh;
	bool too_many = false;
	// the frame-aligned blocks that intersect the region's rects grown by `grow` pixels each way, each once, in raster order
	// (always inlined: left out of line, its scan would reload tiles_x through the closure for every block)
	auto aligned_blocks = [&](uint64_t grow) __attribute__((always_inline)) {
		std::vector<uint8_t> hit(tiles_x * tiles_y, 0);
		for (uint32_t i = 0; i < n_region; i++) {
			const rmd_tile_rect &r = region[i];
			if (r.width == 0 || r.height == 0) continue;
			const uint64_t x0 = r.left > grow ? r.left - grow : 0u, y0 = r.top > grow ? r.top - grow : 0u; // (inclusive)
			const uint64_t x1 = std::min<uint64_t>(width, (uint64_t)r.left + r.width + grow), y1 = std::min<uint64_t>(height, (uint64_t)r.top + r.height + grow); // (exclusive)
			for (uint64_t by = y0 / bh; by <= (y1 - 1u) / bh; by++) std::fill(hit.begin() + by * tiles_x + x0 / bw, hit.begin() + by * tiles_x + (x1 - 1u) / bw + 1u, (uint8_t)1);
		}
		for (uint64_t by = 0; by < tiles_y; by++)
			for (uint64_t bx = 0; bx < tiles_x; bx++)
				if (hit[by * tiles_x + bx]) table.push_back(DualBlock{(uint32_t)(bx * bw), (uint32_t)(by * bh), width, height});
	};
	// the region's rects cut into blocks from their own corners, each entry with its rect's far corner
	auto region_blocks = [&] {
		for (uint32_t i = 0; i < n_region; i++) {
			const rmd_tile_rect &r = region[i];
			const uint64_t n = (((uint64_t)r.width + bw - 1u) / bw) * (((uint64_t)r.height + bh - 1u) / bh);
			if (table.size() + n > 0x7fffffffu) return void(too_many = true);
			for (uint32_t y = 0; y < r.height; y += bh)
				for (uint32_t x = 0; x < r.width; x += bw) table.push_back(DualBlock{r.left + x, r.top + y, r.left + r.width, r.top + r.height});
		}
	};
	if (tiles_x * tiles_y > 0x7fffffffu) return T.too_large = AtrousRegionTables::kFrameTooLarge, T;
	for (uint32_t t = 0; t <= levels && !too_many; t++) {
		T.first[t] = (uint32_t)table.size();
		if (t == levels) region_blocks(); // the last level; at levels = 0 the prologue and the closed form
		else aligned_blocks(t == 0 ? 2u * ((1ull << levels) - 1u) : 2u * ((1ull << levels) - (1ull << t))); // (table t > 0 is level t - 1's: R_{t-1})
		T.count[t] = (uint32_t)(table.size() - T.first[t]);
		if (table.size() > 0x7fffffffu) too_many = true;
	}
	if (too_many) T.too_large = AtrousRegionTables::kRegionTooLarge;
	return T;
}

} // namespace rmd
