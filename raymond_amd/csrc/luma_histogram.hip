// The luminance histogram over tile rectangles (rmd_luminance_histogram_tiles; include/raymond_hip.h states the definition, DESIGN.md section 23 the
// structure).  A translation unit of its own: no other unit's code objects change.
//
// luma_histogram_kernel<DUAL> — one workgroup per ResolveRun (resolve_tiles_host.hpp: rmd_resolve_tonemap_tiles's table): at most 1024 consecutive packed
//                               pixels of ONE rect.  Lane t takes the run's pixels t, t + 256, t + 512, t + 768 — neighbouring lanes read neighbouring
//                               pixels' 24 bytes (48 with DUAL: the second sum buffer, added in one rounded addition) —, divides by the rect's count,
//                               takes luma_bins.hpp's luminance and counter, and counts in 261 words of LDS.  A wave's 64 lanes often hold the SAME counter
//                               (a black wall, a lit ceiling) and same-address LDS atomics serialise, so the wave aggregates first: it walks its distinct
//                               counters — readfirstlane of a still-pending lane's counter, a ballot of the lanes that hold it — and one lane adds the
//                               ballot's population.  After a barrier the workgroup adds its non-zero words to the call's 261 uint64 in global memory.
// The run's eight words are the same for every lane of the workgroup: scalar loads.  f64 throughout, built with -ffp-contract=off like the rest.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "luma_bins.hpp"
#include "resolve_tiles_host.hpp"

namespace rmd {

constexpr uint32_t kLumaLanes = 256u, kLumaNone = 0xFFFFFFFFu;
static_assert(kLumaLanes * kResolveGroup == kResolveRun, "256 lanes x 4 pixels cover one run");

template <bool DUAL>
__global__ __launch_bounds__(256) void luma_histogram_kernel(const double *__restrict__ accum, const double *__restrict__ accum2, uint32_t W,
                                                              const ResolveRun *__restrict__ runs, unsigned long long *__restrict__ counters) {
	__shared__ uint32_t local[kLumaCounters];
	for (uint32_t i = threadIdx.x; i < kLumaCounters; i += kLumaLanes) local[i] = 0u;
	__syncthreads();
	const ResolveRun r = runs[blockIdx.x];
	const double sc = (double)r.samples;
	const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
	for (uint32_t k = 0; k < kResolveGroup; k++) {
		const uint32_t q = k * kLumaLanes + threadIdx.x; // the pixel inside the run; r.n <= 1024
		uint32_t counter = kLumaNone;
		if (q < r.n) {
			const uint32_t at = r.local + q;
			const uint32_t x = at % r.width, y = at / r.width;
			const size_t i = ((size_t)(r.left + x) + (size_t)(r.top + y) * W) * 3;
			double p[3];
#pragma unroll
			for (int c = 0; c < 3; c++) {
				const double s = DUAL ? accum[i + c] + accum2[i + c] : accum[i + c];
				p[c] = s / sc; // TaskHandle::await, src/trace.rs:95
			}
			counter = luma_counter(luma_bits(luma_of(p[0], p[1], p[2])));
		}
		// one LDS add per distinct counter of the wave: each trip retires every lane that holds the first pending lane's counter
		bool pending = counter != kLumaNone;
		while (pending) {
			const uint32_t first = __builtin_amdgcn_readfirstlane(counter);
			const unsigned long long same = __ballot(counter == first); // (of the lanes still in the loop)
			if (counter == first) {
				if ((same & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&local[first], (uint32_t)__popcll(same));
				pending = false;
			}
		}
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < kLumaCounters; i += kLumaLanes) {
		const uint32_t n = local[i];
		if (n != 0u) atomicAdd(&counters[i], (unsigned long long)n);
	}
}

hipError_t launch_luma_histogram(hipStream_t stream, const double *accum, const double *accum2, uint32_t W, const ResolveRun *runs, uint32_t n_runs,
                                 uint64_t *counters) {
	if (n_runs == 0) return hipSuccess;
	unsigned long long *out = reinterpret_cast<unsigned long long *>(counters);
	if (accum2) hipLaunchKernelGGL(luma_histogram_kernel<true>, dim3(n_runs), dim3(kLumaLanes), 0, stream, accum, accum2, W, runs, out);
	else hipLaunchKernelGGL(luma_histogram_kernel<false>, dim3(n_runs), dim3(kLumaLanes), 0, stream, accum, accum2, W, runs, out);
	return hipGetLastError();
}

} // namespace rmd
