// Closest-hit queries for caller-supplied rays (rmd_intersect_rays, rmd_camera_rays; include/raymond_hip.h states the definition, DESIGN.md
// section 36 the structure and its cost).  A translation unit of its own: no other code object changes.
//
// rays_kernel<GRID> — a wave serves batches of 64 consecutive rays, lane = ray (rays_plan.hpp: wave u takes batches u, u + total_waves, ...).  Per
// batch: the lane's ray, Scene::intersect on it (scene_intersect_wave, render_kernel.hpp: all 64 lanes are in every call because the grids' walk is
// wave-cooperative, `want` marking the lanes whose ray exists), the normal rmd_render_features defines, and the lane's 40-byte record.  Rays are
// independent and nothing is shared between batches, so a record depends on its ray alone, whatever the plan.
// The workgroup is first_hit_body's (first_hit.hpp): the one-wave-per-item form of the render's launch plan, [object table][grid occupancy masks]
// [one area per wave], staged by stage_scene_tables and one barrier.  The table is read from LDS for the normals.
// The rays are any caller's: `arbitrary_rays` sends every axis pair down its general test (scene_split.hpp: axis_pair_test).  The object loop's
// turns are the scene's visit_mask: it is made once at scene upload from the objects alone (api_scene.cpp: derive_scene_objects) and clears only
// planes marked kPairTestedAtPartner, which the loops pass by for every ray — so it holds for rays that are not a launch's own.
// f64 throughout, built with -ffp-contract=off like the rest of the library.
#include "first_hit.hpp"
#include "rays_plan.hpp"

namespace rmd {

static_assert(sizeof(rmd_ray_hit) == 40 && RMD_HIT_DOUBLES * sizeof(double) == sizeof(rmd_ray_hit) && RMD_RAY_DOUBLES == 6, "the layouts of include/raymond_hip.h");
static_assert(RMD_MAX_RAYS == RMD_RAYS_MAX_RAYS, "rays_plan.hpp mirrors include/raymond_hip.h");

typedef double Pair64 __attribute__((ext_vector_type(2))); // 16 bytes, 16-byte aligned: one global_store of four dwords

// The lane's ray: 48 contiguous bytes, a wave's 64 are 3,072.  Six doubles read in a row: the compiler makes three 16-byte loads a lane of them whatever
// the buffer's alignment (this target's vector memory instructions take unaligned addresses), so no aligned form is written out.
RMD_DEV void load_ray(const double *__restrict__ rays, size_t i, V3 &ro, V3 &rd) {
	const RMD_GLOBAL double *r = as_global(rays + i * RMD_RAY_DOUBLES);
	ro = ld3(r), rd = ld3(r + 3);
}

// The lane's record: 40 bytes at a 40-byte stride, so every other record begins 8 bytes past a 16-byte boundary.  One 8-byte and two 16-byte
// stores either way, without a branch: a record on a boundary is [16][16][8], the others [8][16][16].  d4 = the object and triangle words.
RMD_DEV void store_hit(rmd_ray_hit *__restrict__ hits, size_t i, double d0, double d1, double d2, double d3, double d4) {
	RMD_GLOBAL double *h = (RMD_GLOBAL double *)(reinterpret_cast<double *>(hits) + i * RMD_HIT_DOUBLES);
	const bool odd = ((uintptr_t)h & 8u) != 0u;
	h[odd ? 0 : 4] = odd ? d0 : d4;
	RMD_GLOBAL Pair64 *q = (RMD_GLOBAL Pair64 *)(h + (odd ? 1 : 0));
	q[0] = odd ? Pair64{d1, d2} : Pair64{d0, d1};
	q[1] = odd ? Pair64{d3, d4} : Pair64{d2, d3};
}

template <bool GRID>
__global__ __launch_bounds__(GRID ? 64 * kGridWavesPerWg : 64) void rays_kernel(RenderParams P, const DevObject *__restrict__ objs, const DevGrid *__restrict__ grids,
                                                                                 uint32_t wave_lds, const double *__restrict__ rays, uint32_t n_rays,
                                                                                 uint32_t n_batches, uint32_t total_waves, rmd_ray_hit *__restrict__ hits) {
	extern __shared__ __align__(16) unsigned char smem[];
	DevObject *lobjs = reinterpret_cast<DevObject *>(smem);
	uint32_t *lmasks = reinterpret_cast<uint32_t *>(smem + (size_t)P.n_objects * sizeof(DevObject));
	const uint32_t tid = threadIdx.x, wave = tid >> 6, waves_per_wg = blockDim.x >> 6, lane = tid & 63u;
	stage_scene_tables<GRID>(P, objs, grids, lobjs, lmasks);
	__syncthreads(); // the only workgroup barrier: from here on every wave runs on its own
	const uint32_t *lds_masks = P.mask_words_total ? lmasks : nullptr;
	WalkScratch &scr = *reinterpret_cast<WalkScratch *>(smem + (size_t)P.n_objects * sizeof(DevObject) + (size_t)((P.mask_words_total + 3u) & ~3u) * 4u +
	                                                    (size_t)wave * wave_lds); // (never touched without a grid)

	// the wave's batches (rays_plan.hpp): a trip count made of scalars, every lane of the wave in every trip
	const uint32_t unit = __builtin_amdgcn_readfirstlane(blockIdx.x * waves_per_wg + wave);
	for (uint32_t b = unit; b < n_batches; b += total_waves) {
		const uint32_t i = b * kRaysBatch + lane; // (< 2^30 + 64)
		const bool want = i < n_rays;
		V3 ro, rd;
		load_ray(rays, want ? i : 0u, ro, rd); // (a lane past the end reads ray 0, which exists, and keeps nothing of it)
		double t = 0.0;
		uint32_t sub = 0;
		const int oi = scene_intersect_wave<GRID>(objs, P.n_objects, grids, lds_masks, scr, want, ro, rd, t, sub, P.axis_pairs, 0u, nullptr, /*arbitrary_rays=*/true, P.visit_mask);
		const bool hit = want && oi >= 0;
		V3 normal = mk(0.0, 0.0, 0.0);
		if (hit) { // FeatureSink::add's normal (features.hip)
			const DevObject &o = lobjs[oi];
			const V3 frag = ro + rd * t; // :246
			if (o.geometry_kind == 0u) normal = ld3(o.normal);                        // plane.rs:28-32 (as stored)
			else if (o.geometry_kind == 1u) normal = normalize(frag - ld3(o.origin)); // sphere.rs:31-35
			else if constexpr (GRID) {
				const DevGrid &g = grids[o.grid_index];
				normal = triangle_normal(as_global(g.tri_pos) + (size_t)sub * 9, as_global(g.tri_nrm) + (size_t)sub * 9, as_global(g.tri_aux) + (size_t)sub * 4, frag); // acc_grid.rs:85-87
			}
		}
		// a miss is {0, {0, 0, 0}, -1, 0} in full; `sub` is 0 for a plane or a sphere (scene_intersect_wave)
		const unsigned long long words = hit ? ((unsigned long long)(uint32_t)oi | (unsigned long long)sub << 32) : 0xFFFFFFFFull;
		if (want) store_hit(hits, i, hit ? t : 0.0, normal.x, normal.y, normal.z, __builtin_bit_cast(double, words));
	}
}

// rmd_camera_rays: one lane per entry, the pinhole generate_primary_ray (device_core.hpp: primary_ray) of pixel xy[2i], xy[2i + 1] at the jitter
// uniforms uv[2i], uv[2i + 1] — 0.5, 0.5, the pixel's centre, without uv
__global__ __launch_bounds__(256) void camera_rays_kernel(RenderParams P, const uint32_t *__restrict__ xy, const double *__restrict__ uv, uint32_t n,
                                                           double *__restrict__ rays) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const double u0 = uv ? uv[2 * (size_t)i] : 0.5, u1 = uv ? uv[2 * (size_t)i + 1] : 0.5;
	V3 ro, rd;
	primary_ray(P, xy[2 * (size_t)i], xy[2 * (size_t)i + 1], u0, u1, ro, rd);
	double *r = rays + (size_t)i * RMD_RAY_DOUBLES;
	r[0] = ro.x, r[1] = ro.y, r[2] = ro.z, r[3] = rd.x, r[4] = rd.y, r[5] = rd.z;
}

// What the launch of rmd_intersect_rays on this scene would be: the render plan's one-wave-per-item workgroup (as launch_first_hit takes it) and
// rays_plan.hpp's waves.  *lds and *wave_lds may be null.  False: the scene's tables do not fit (never after check_scene_fits: api_rays.cpp)
bool plan_rays_launch(const RenderParams &P, uint64_t n_rays, uint32_t n_cus, RaysPlan &plan, size_t *lds, size_t *wave_lds) {
	const bool grid = P.n_grids != 0u;
	const LaunchPlan L = plan_render_launch(kModeTiles, grid, P.n_objects, P.mask_words_total, false, false, false, false, 1u, 0u);
	if (L.lds > kLdsBudgetBytes || L.waves_per_wg == 0u || L.waves_per_wg > (grid ? kGridWavesPerWg : 1u)) return false;
	plan = rays_plan(n_rays, n_cus, L.waves_per_wg);
	if (lds) *lds = L.lds;
	if (wave_lds) *wave_lds = L.wave_lds;
	return true;
}

hipError_t launch_rays(hipStream_t stream, const RenderParams &P, const DevObject *objs, const DevGrid *grids, uint32_t n_cus, const double *rays, uint64_t n_rays,
                       rmd_ray_hit *hits) {
	if (n_rays == 0u) return hipSuccess;
	if (n_rays > RMD_MAX_RAYS) return hipErrorInvalidValue; // (never: the caller refuses it)
	RaysPlan plan;
	size_t lds = 0, wave_lds = 0;
	if (!plan_rays_launch(P, n_rays, n_cus, plan, &lds, &wave_lds)) return hipErrorInvalidConfiguration;
	const auto kernel = P.n_grids != 0u ? &rays_kernel<true> : &rays_kernel<false>;
	if (lds > 64u * 1024u) {
		hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudgetBytes);
		if (e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(kernel, dim3(plan.workgroups), dim3(64u * plan.waves_per_wg), lds, stream, P, objs, grids, (uint32_t)wave_lds, rays, (uint32_t)n_rays, plan.batches,
	                   plan.total_waves, hits);
	return hipGetLastError();
}

hipError_t launch_camera_rays(hipStream_t stream, const RenderParams &P, const uint32_t *xy, const double *uv, uint64_t n_rays, double *rays) {
	if (n_rays == 0u) return hipSuccess;
	if (n_rays > RMD_MAX_RAYS) return hipErrorInvalidValue; // (never: the caller refuses it)
	hipLaunchKernelGGL(camera_rays_kernel, dim3((uint32_t)((n_rays + 255u) / 256u)), dim3(256), 0, stream, P, xy, uv, (uint32_t)n_rays, rays);
	return hipGetLastError();
}

} // namespace rmd
