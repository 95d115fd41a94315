// The summation order of the per-tile measures (rmd_tile_luma_error, rmd_tile_weighted_error), written once: 256 lanes, lane t taking the rect's row-major
// pixels t, t + 256, ...; within each wave of 64 the exchange with the lane 32, 16, 8, 4, 2, 1 apart; then the four waves' sums as (w0 + w1) + (w2 + w3).
// That order is why a measure's bits do not depend on scheduling, and the kernels (tile_luma.hip, tile_weighted.hip), the host emulations of the rule
// headers, the C++ mirror and the rule mains under tests/ all take it from here; tests/tile_reduce_ref.py restates it.  Needs only <stdint.h>; under hipcc
// the functions are __host__ __device__ and the combine is there, for which a unit built by hipcc includes <hip/hip_runtime.h> before this header.  Built
// without contraction (-ffp-contract=off) wherever it is built.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RMD_LUMA_HD __host__ __device__
#else
#define RMD_LUMA_HD
#endif

namespace rmd {

constexpr uint32_t kTileLanes = 256u, kTileWave = 64u; // one workgroup of four waves per rect
static_assert(kTileLanes == 4u * kTileWave && kTileWave == 64u, "the combines below are written for four waves of 64");

// What a lane carries, and what the combine adds: the sums of Y, V and the rule's own term E (tile_luma_rule.hpp: R; tile_weighted_rule.hpp: the weighted
// variance) over valid pixels, and the two counts
struct TileSums {
	double sy = 0.0, sv = 0.0, se = 0.0;
	uint32_t valid = 0u, invalid = 0u;
};
RMD_LUMA_HD inline TileSums tile_sums_add(const TileSums &a, const TileSums &b) {
	TileSums o;
	o.sy = a.sy + b.sy, o.sv = a.sv + b.sv, o.se = a.se + b.se;
	o.valid = a.valid + b.valid, o.invalid = a.invalid + b.invalid;
	return o;
}

// The frame index of pixel i (row-major) of the rect at (left, top), `width` wide, in a frame `frame_width` wide
RMD_LUMA_HD inline uint64_t tile_pixel_index(uint64_t i, uint32_t left, uint32_t top, uint32_t width, uint32_t frame_width) {
	return (uint64_t)(left + (uint32_t)(i % width)) + (uint64_t)(top + (uint32_t)(i / width)) * frame_width;
}

#if defined(__HIPCC__)
// Device only, called by all 256 threads of a workgroup: the lanes' sums meet by __shfl_xor within each wave, lane 0 of each wave leaves them in LDS, and
// after the barrier thread 0 adds the four waves'.  True for thread 0 alone, whose `a` is then the rect's sums.  (static: the two LDS arrays are then each
// kernel's own, laid out with its other LDS as if declared in it.  Each field meets its partner's right after the exchange, tile_sums_add's sums in the
// kernels' instruction order)
static __device__ inline bool tile_sums_combine(TileSums &a) {
	for (int off = 32; off > 0; off >>= 1) {
		a.sy = a.sy + __shfl_xor(a.sy, off, 64), a.sv = a.sv + __shfl_xor(a.sv, off, 64), a.se = a.se + __shfl_xor(a.se, off, 64);
		a.valid += __shfl_xor(a.valid, off, 64), a.invalid += __shfl_xor(a.invalid, off, 64);
	}
	__shared__ double wave_sum[3][4];
	__shared__ uint32_t wave_count[2][4];
	if ((threadIdx.x & 63u) == 0u) {
		const uint32_t w = threadIdx.x >> 6;
		wave_sum[0][w] = a.sy, wave_sum[1][w] = a.sv, wave_sum[2][w] = a.se;
		wave_count[0][w] = a.valid, wave_count[1][w] = a.invalid;
	}
	__syncthreads();
	if (threadIdx.x != 0u) return false;
	a.sy = (wave_sum[0][0] + wave_sum[0][1]) + (wave_sum[0][2] + wave_sum[0][3]);
	a.sv = (wave_sum[1][0] + wave_sum[1][1]) + (wave_sum[1][2] + wave_sum[1][3]);
	a.se = (wave_sum[2][0] + wave_sum[2][1]) + (wave_sum[2][2] + wave_sum[2][3]);
	a.valid = (wave_count[0][0] + wave_count[0][1]) + (wave_count[0][2] + wave_count[0][3]);
	a.invalid = (wave_count[1][0] + wave_count[1][1]) + (wave_count[1][2] + wave_count[1][3]);
	return true;
}
#endif

// Host only.  One rect as the kernel walks it: 256 emulated lanes, each meeting its pixels in the kernel's order, then the kernel's combine.
// add(sums, pix): the rule's per-pixel step on the frame's pixel `pix`; the rect lies inside the frame
template <class Add>
inline TileSums tile_rect_sums_host(uint32_t frame_width, uint32_t left, uint32_t top, uint32_t width, uint32_t height, Add add) {
	TileSums lane[kTileLanes];
	const uint64_t n_px = (uint64_t)width * height;
	for (uint32_t t = 0; t < kTileLanes; t++)
		for (uint64_t i = t; i < n_px; i += kTileLanes) add(lane[t], tile_pixel_index(i, left, top, width, frame_width));
	for (uint32_t off = kTileWave / 2u; off > 0u; off >>= 1) {
		TileSums next[kTileLanes];
		for (uint32_t t = 0; t < kTileLanes; t++) next[t] = tile_sums_add(lane[t], lane[t ^ off]); // (t ^ off stays inside t's wave: off < 64)
		for (uint32_t t = 0; t < kTileLanes; t++) lane[t] = next[t];
	}
	return tile_sums_add(tile_sums_add(lane[0], lane[kTileWave]), tile_sums_add(lane[2u * kTileWave], lane[3u * kTileWave]));
}

} // namespace rmd
