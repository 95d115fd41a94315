// The rule of the AO buffers (rmd_render_ao, rmd_ao_resolve; include/raymond_hip.h states the definition): the lines the kernels (ao.hip), the C++
// mirror (raymond_amd/host) and tests/ao_rule_main.cpp all read.  Needs only <stdint.h>; under hipcc the functions are __host__ __device__.  Integers
// throughout but for the resolve's one division.  In the kernel the four words of a record are four registers: every index is a constant.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RMD_AO_HD __host__ __device__
#else
#define RMD_AO_HD
#endif

namespace rmd {

constexpr uint32_t kAoWords = 4u; // RMD_AO_WORDS: occluded open none samples
constexpr uint32_t kAoOccluded = 0u, kAoOpen = 1u, kAoNone = 2u, kAoSamples = 3u;

// One sample: without a first hit (a miss, or no ray) it is `none`; with one it is `occluded` or `open`; then `samples`.  Counts wrap at 2^32
RMD_AO_HD inline void ao_count(uint32_t rec[kAoWords], bool first_hit, bool occluded) {
	rec[0] += (first_hit && occluded) ? 1u : 0u;
	rec[1] += (first_hit && !occluded) ? 1u : 0u;
	rec[2] += first_hit ? 0u : 1u;
	rec[3] += 1u;
}

// The openness of one pixel: open over open + occluded (a 64-bit sum), one division; `empty_value` for a pixel without a first hit.
// *empty (never null) is whether the pixel is such a one
RMD_AO_HD inline double ao_resolve_pixel(const uint32_t rec[kAoWords], double empty_value, bool *empty) {
	const uint64_t den = (uint64_t)rec[1] + (uint64_t)rec[0];
	*empty = den == 0u;
	return den == 0u ? empty_value : (double)rec[1] / (double)den;
}

} // namespace rmd
