// A tile's variance weighted by its pixels' luminance (rmd_tile_weighted_error; include/raymond_hip.h states the definition, DESIGN.md section 30 the
// structure).  A translation unit of its own: no other unit's code objects change.  The rule — a pixel's validity, Y and V (despike_rule.hpp), its counter
// (luma_bins.hpp), the weighted variance, the final step — is tile_weighted_rule.hpp's, which the C++ mirror and tests/tile_weighted_rule_main.cpp read as
// well.
//
// tile_weighted_kernel — one workgroup of 256 threads (four waves of 64) per rect:
//   0. the 260 weights go from global memory into LDS once (2,080 B): thread t takes entry t, threads 0 - 3 also entries 256 - 259; one barrier;
//   1. lane t takes the rect's row-major pixels t, t + 256, ...: 2 x 24 bytes a pixel, neighbouring lanes neighbouring records; a pixel's weight is the
//      LDS entry its luminance's bits name — no transcendental function, one product —; the lane keeps the sums of Y, V and E over its valid pixels and
//      counts the valid and the invalid ones;
//   2. tile_reduce.hpp's combine: within a wave the five values meet by the xor exchange over 32, 16, 8, 4, 2, 1; lane 0 of each wave leaves them in LDS;
//      thread 0 adds the four waves' as (w0 + w1) + (w2 + w3);
//   3. thread 0 takes the final step and writes the rect's 40 bytes with plain stores.
// No atomics: the bits do not depend on scheduling.  f64 throughout, built with -ffp-contract=off like the rest of the library.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "tile_weighted_rule.hpp"

namespace rmd {

static_assert(kLumaWeights == kTileLanes + 4u, "the copy below is written for 256 + 4 weights");

__global__ __launch_bounds__(256) void tile_weighted_kernel(const double *__restrict__ S, const double *__restrict__ Q, const rmd_tile_rect *__restrict__ rects,
                                                             const uint32_t *__restrict__ counts, uint32_t W, const double *__restrict__ weights,
                                                             TileWeighted *__restrict__ out) {
	__shared__ double lds_weights[kLumaWeights];
	lds_weights[threadIdx.x] = weights[threadIdx.x];
	if (threadIdx.x < kLumaWeights - 256u) lds_weights[256u + threadIdx.x] = weights[256u + threadIdx.x];
	__syncthreads();
	const rmd_tile_rect r = rects[blockIdx.x];
	const uint32_t n = counts[blockIdx.x];
	const uint64_t n_px = (uint64_t)r.width * r.height;
	TileSums a;
	for (uint64_t i = threadIdx.x; i < n_px; i += kTileLanes) {
		const size_t pix = tile_pixel_index(i, r.left, r.top, r.width, W);
		double s[3], q[3];
#pragma unroll
		for (int c = 0; c < 3; c++) s[c] = S[pix * 3 + c], q[c] = Q[pix * 3 + c];
		tile_weighted_add(a, s, q, n, lds_weights);
	}
	if (tile_sums_combine(a)) out[blockIdx.x] = tile_weighted_final(a.sy, a.sv, a.se, a.valid, a.invalid, n_px);
}

hipError_t launch_tile_weighted(hipStream_t stream, const DenoiseInput &in, const double *weights, TileWeighted *out) {
	if (in.n_rects == 0u) return hipSuccess;
	hipLaunchKernelGGL(tile_weighted_kernel, dim3(in.n_rects), dim3(256), 0, stream, in.accum_a, in.accum_sq_a, in.rects, in.counts_a, in.W, weights, out);
	return hipGetLastError();
}

} // namespace rmd
