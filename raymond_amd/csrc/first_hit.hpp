// The first-hit passes' shared device body and launcher (rmd_render_features: features.hip; rmd_render_ids: ids.hip, section 34;
// rmd_render_ao: ao.hip, section 35).
// A pass is a sink — what a lane keeps of a sample's first hit, and the buffers it loads and stores — around the one body below.
//
// first_hit_body<GRID> — one wave per 8 x 8 wave tile, lane = pixel.  For each sample of the call, in order: the primary ray exactly as the render
// takes it (block 0 = the jitter, then the thin lens' rounds), Scene::intersect on it once (scene_intersect_wave, render_kernel.hpp: the grids'
// wave-cooperative walk, so all 64 lanes stay in the sample loop and in every call, `want` marking the lanes that carry a ray), and the hit — a miss,
// or a sample the thin lens yields no ray for, is no hit — handed to the sink.  The sink's state is read once, kept in registers and written once:
// it is sequential in sample order whatever the rects, so [0, k) + [k, n) is [0, n) bit for bit.
// The workgroup is the one-wave-per-item form of the render's launch plan (launch.hpp: plan_render_launch, direct mode): [object table]
// [grid occupancy masks][one area per wave], of which a wave uses the walk scratch.
// f64 throughout, built with -ffp-contract=off like the rest of the library.
//
// A sink offers
//   load(alive, pixel)                                  the lane's state from its buffers (pixel = x + y * W; a lane that is not alive reads nothing)
//   add<GRID>(hit, oi, lobjs, grids, ro, rd, t, sub)    one sample; called by all 64 lanes, `hit` false for a miss and for a lane without a ray
//   store(pixel)                                        the state back; called only where alive
// A sink that declares `static constexpr bool kSecondRay = true` follows one more segment per sample (rmd_render_ao: ao.hip) and also offers
//   second_ray(P, rng, origin, dir) -> want2            after add: the follow-up ray of the lane's sample — rng stands at the sample's next block —, want2 false where
//                                                       the lane has none; called by all 64 lanes
//   second_hit(hit2, t2)                                what Scene::intersect gave on it (the same wave-cooperative call, want2 marking the lanes); hit2 false for a
//                                                       miss and for a lane without a follow-up ray; called by all 64 lanes
// The other sinks' kernels hold none of this.
#pragma once
#include <type_traits>

#include "render_kernel.hpp"

namespace rmd {

template <class Sink, class = void>
struct sink_second_ray : std::false_type {};
template <class Sink>
struct sink_second_ray<Sink, std::void_t<decltype(Sink::kSecondRay)>> : std::bool_constant<Sink::kSecondRay> {};

// Stage the object table and, with grids, their occupancy masks in LDS: coalesced, once per workgroup (the caller's barrier follows).
// render_kernel_body keeps its own copy of these lines: calling this from there changed the render kernels' register allocation, which is at its limit.
template <bool GRID>
RMD_DEV void stage_scene_tables(const RenderParams &P, const DevObject *__restrict__ objs, const DevGrid *__restrict__ grids, DevObject *lobjs, uint32_t *lmasks) {
	const uint32_t tid = threadIdx.x;
	const double *src = reinterpret_cast<const double *>(objs);
	double *dst = reinterpret_cast<double *>(lobjs);
	for (uint32_t i = tid; i < P.n_objects * 16u; i += blockDim.x) dst[i] = src[i];
	if constexpr (GRID) {
		for (uint32_t gi = 0; gi < P.n_grids; gi++) {
			const DevGrid &g = grids[gi];
			if (g.mask_lds_word == 0xFFFFFFFFu) continue;
			for (uint32_t i = tid; i < g.mask_n_words; i += blockDim.x) lmasks[g.mask_lds_word + i] = as_global(g.mask_words)[i];
		}
	}
}

// P is the calling kernel's by-value argument
template <bool GRID, class Sink>
RMD_DEV void first_hit_body(const RenderParams &P, const DevObject *__restrict__ objs, const DevGrid *__restrict__ grids, const WaveTile *__restrict__ tiles,
                            uint32_t wave_lds, Sink &sink) {
	extern __shared__ __align__(16) unsigned char smem[];
	DevObject *lobjs = reinterpret_cast<DevObject *>(smem);
	uint32_t *lmasks = reinterpret_cast<uint32_t *>(smem + (size_t)P.n_objects * sizeof(DevObject));
	const uint32_t tid = threadIdx.x, wave = tid >> 6, waves_per_wg = blockDim.x >> 6, lane = tid & 63u;
	stage_scene_tables<GRID>(P, objs, grids, lobjs, lmasks);
	__syncthreads(); // the only workgroup barrier: from here on every wave runs on its own
	const uint32_t *lds_masks = P.mask_words_total ? lmasks : nullptr;
	WalkScratch &scr = *reinterpret_cast<WalkScratch *>(smem + (size_t)P.n_objects * sizeof(DevObject) + (size_t)((P.mask_words_total + 3u) & ~3u) * 4u +
	                                                    (size_t)wave * wave_lds); // (never touched without a grid)

	const uint32_t unit = blockIdx.x * waves_per_wg + wave;
	if (unit >= P.n_work) return; // (uniform per wave: the last workgroup's waves beyond the last wave tile)
	const WaveTile tile = tiles[unit];
	const uint32_t lx = lane & 7u, ly = lane >> 3;
	const bool alive = lx < tile.w && ly < tile.h;
	const uint32_t x = tile.x0 + lx, y = tile.y0 + ly;
	const size_t pixel = (size_t)x + (size_t)y * P.W;
	sink.load(alive, pixel);

	// the kernel's own loop: sample_count trips, every lane of the wave in it (the walk is wave-cooperative)
	for (uint32_t k = 0; k < P.sample_count; k++) {
		Rng rng;
		rng.init(y * P.W + x, P.sample_begin + k);
		V3 ro, rd;
		double u0, u1;
		rng.next2(P.key0, P.key1, u0, u1); // block 0: the pixel jitter (:326-327)
		primary_ray(P, x, y, u0, u1, ro, rd);
		bool failed = false;
		if (P.use_dof) failed = !thin_lens_from_pinhole(P, ro, rd, rng, ro, rd); // the render's sample is zero there: a miss here
		const bool want = alive && !failed;
		double t = 0.0;
		uint32_t sub = 0;
		const int oi = scene_intersect_wave<GRID>(objs, P.n_objects, grids, lds_masks, scr, want, ro, rd, t, sub, P.axis_pairs, 0u, nullptr, false, P.visit_mask);
		sink.template add<GRID>(want && oi >= 0, oi, lobjs, grids, ro, rd, t, sub);
		if constexpr (sink_second_ray<Sink>::value) {
			V3 ro2, rd2;
			const bool want2 = sink.second_ray(P, rng, ro2, rd2);
			double t2 = 0.0;
			uint32_t sub2 = 0;
			int oi2 = -1;
			if (__builtin_amdgcn_ballot_w64(want2) != 0ull) // (uniform per wave: a wave none of whose lanes has a first hit skips the call)
				oi2 = scene_intersect_wave<GRID>(objs, P.n_objects, grids, lds_masks, scr, want2, ro2, rd2, t2, sub2, P.axis_pairs, 0u, nullptr, false, P.visit_mask);
			sink.second_hit(want2 && oi2 >= 0, t2);
		}
	}

	if (alive) sink.store(pixel);
}

// The launch of a first-hit kernel pair (the instantiation with grids, the one without) over P.n_work wave tiles: the workgroup's size and LDS are
// the render's one-wave-per-item plan for this scene (direct mode, no moments); `out` are the pass's own trailing kernel arguments.
template <class... Out>
hipError_t launch_first_hit(hipStream_t stream, const RenderParams &P,
                            void (*kernel_with_grid)(RenderParams, const DevObject *, const DevGrid *, const WaveTile *, uint32_t, Out...),
                            void (*kernel_without)(RenderParams, const DevObject *, const DevGrid *, const WaveTile *, uint32_t, Out...), const DevObject *objs,
                            const DevGrid *grids, const WaveTile *wave_tiles, Out... out) {
	if (P.n_work == 0u || P.sample_count == 0u) return hipSuccess;
	const bool grid = P.n_grids != 0u;
	const LaunchPlan L = plan_render_launch(kModeTiles, grid, P.n_objects, P.mask_words_total, false, false, false, false, P.n_work, 0u);
	if (L.lds > kLdsBudgetBytes || L.waves_per_wg == 0u || L.waves_per_wg > (grid ? kGridWavesPerWg : 1u)) return hipErrorInvalidConfiguration; // (never: check_render_args)
	const auto kernel = grid ? kernel_with_grid : kernel_without;
	if (L.lds > 64u * 1024u) {
		hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudgetBytes);
		if (e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(kernel, dim3(L.workgroups), dim3(64u * L.waves_per_wg), L.lds, stream, P, objs, grids, wave_tiles, (uint32_t)L.wave_lds, out...);
	return hipGetLastError();
}

} // namespace rmd
