// The displayed error of the FILTERED frame (rmd_tile_weighted_error_dual; include/raymond_hip.h states the definition, DESIGN.md section 31 the
// structure).  A translation unit of its own: no other unit's code objects change.  The rule — a pixel's validity, the luminance of its filtered means,
// its counter (luma_bins.hpp), the weighted term and the final step (tile_weighted_rule.hpp) — is tile_weighted_dual_rule.hpp's, which the C++ mirror and
// tests/tile_weighted_dual_rule_main.cpp read as well.
//
// tile_weighted_dual_kernel — one workgroup of 256 threads (four waves of 64) per rect:
//   0. the 260 weights go from global memory into LDS once (2,080 B), as tile_weighted_kernel copies them; one barrier;
//   1. lane t takes the rect's row-major pixels t, t + 256, ...: 24 bytes of the filtered frame and 8 of the error image a pixel, neighbouring lanes
//      neighbouring records; the lane keeps the sums of Y, err and E over its valid pixels and counts the valid and the invalid ones;
//   2. tile_reduce.hpp's combine;
//   3. thread 0 takes the final step and writes the rect's 40 bytes with plain stores.
// No atomics: the bits do not depend on scheduling.  f64 throughout, built with -ffp-contract=off like the rest of the library.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "tile_weighted_dual_rule.hpp"

namespace rmd {

static_assert(kLumaWeights == kTileLanes + 4u, "the copy below is written for 256 + 4 weights");

__global__ __launch_bounds__(256) void tile_weighted_dual_kernel(const double *__restrict__ out_img, const double *__restrict__ err, const rmd_tile_rect *__restrict__ rects,
                                                                  uint32_t W, const double *__restrict__ weights, TileWeighted *__restrict__ out) {
	__shared__ double lds_weights[kLumaWeights];
	lds_weights[threadIdx.x] = weights[threadIdx.x];
	if (threadIdx.x < kLumaWeights - 256u) lds_weights[256u + threadIdx.x] = weights[256u + threadIdx.x];
	__syncthreads();
	const rmd_tile_rect r = rects[blockIdx.x];
	const uint64_t n_px = (uint64_t)r.width * r.height;
	TileSums a;
	for (uint64_t i = threadIdx.x; i < n_px; i += kTileLanes) {
		const size_t pix = tile_pixel_index(i, r.left, r.top, r.width, W);
		double o[3];
#pragma unroll
		for (int c = 0; c < 3; c++) o[c] = out_img[pix * 3 + c];
		tile_weighted_dual_add(a, o, err[pix], lds_weights);
	}
	if (tile_sums_combine(a)) out[blockIdx.x] = tile_weighted_final(a.sy, a.sv, a.se, a.valid, a.invalid, n_px);
}

hipError_t launch_tile_weighted_dual(hipStream_t stream, const double *out_img, const double *err, const rmd_tile_rect *rects, uint32_t n_rects, uint32_t W,
                                     const double *weights, TileWeighted *out) {
	if (n_rects == 0u) return hipSuccess;
	hipLaunchKernelGGL(tile_weighted_dual_kernel, dim3(n_rects), dim3(256), 0, stream, out_img, err, rects, W, weights, out);
	return hipGetLastError();
}

} // namespace rmd
