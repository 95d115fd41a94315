// The launch plan of rmd_intersect_rays (rays.hip): how n rays become batches, waves and workgroups.  Pure host arithmetic,
// <stdint.h> only: read by the launcher (rays.hip), the host library's callers (api_rays.cpp), the C++ mirror's tests and a stand-alone program
// (tests/rays_plan_main.cpp) that checks it under the sanitizers.
//
// A batch is 64 consecutive rays, lane = ray: batch b holds rays [64 b, 64 b + 64).  A wave serves batches; staging the scene's tables costs a
// workgroup up to 150 KB of loads, so a launch has no more waves than fill the device kRaysFill times over and a wave loops: wave u of the
// total_waves launched takes batches u, u + total_waves, u + 2 total_waves, ...  — rays_plan_trips(plan, u) of them, a number every lane of the wave
// computes from the same scalars.
#pragma once
#include <stdint.h>

#define RMD_RAYS_MAX_RAYS (1ull << 30) /* include/raymond_hip.h: RMD_MAX_RAYS — 64 * batches and a ray's index stay below 2^31 */

namespace rmd {

constexpr uint32_t kRaysBatch = 64u;      // rays of a batch: one per lane
constexpr uint32_t kRaysSlotsPerCu = 16u; // wave slots of a CU at 4 waves per SIMD
constexpr uint32_t kRaysFill = 4u;        // times over a launch may fill the device's wave slots before its waves loop

struct RaysPlan {
	uint32_t batches = 0;      // ceil(n_rays / 64)
	uint32_t waves_per_wg = 0; // the render plan's one-wave-per-item form for the scene (launch.hpp: plan_render_launch)
	uint32_t workgroups = 0;   // 0: no launch (n_rays == 0)
	uint32_t total_waves = 0;  // workgroups * waves_per_wg: the stride of the batch loop (the last workgroup's spare waves have no batch)
};

// n_rays <= RMD_RAYS_MAX_RAYS (the caller refuses more); n_cus and waves_per_wg of 0 count as 1.
inline RaysPlan rays_plan(uint64_t n_rays, uint32_t n_cus, uint32_t waves_per_wg) {
	RaysPlan p;
	if (n_cus == 0u) n_cus = 1u;
	if (waves_per_wg == 0u) waves_per_wg = 1u;
	p.waves_per_wg = waves_per_wg;
	const uint64_t batches = (n_rays + (kRaysBatch - 1u)) / kRaysBatch;
	p.batches = (uint32_t)batches;
	if (batches == 0u) return p;
	const uint64_t cap = (uint64_t)n_cus * kRaysSlotsPerCu * kRaysFill; // waves that fill the device kRaysFill times over
	const uint64_t waves = batches < cap ? batches : cap;
	const uint64_t wgs = (waves + waves_per_wg - 1u) / waves_per_wg;
	p.workgroups = (uint32_t)wgs;
	p.total_waves = (uint32_t)(wgs * waves_per_wg);
	return p;
}

// Batches wave `wave` (0 .. total_waves - 1) takes: wave, wave + total_waves, ...  below p.batches
inline uint32_t rays_plan_trips(const RaysPlan &p, uint32_t wave) {
	if (p.total_waves == 0u || wave >= p.batches) return 0u;
	return (p.batches - wave + p.total_waves - 1u) / p.total_waves;
}

} // namespace rmd
