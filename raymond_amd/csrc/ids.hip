// First-hit object IDs with coverage, and mattes from them (rmd_render_ids, rmd_ids_matte; include/raymond_hip.h states the definition, ids_rule.hpp
// the rule, DESIGN.md section 34 the structure and its cost).  A translation unit of its own: no other unit's code objects change.
//
// ids_kernel<GRID> — features_kernel<GRID>'s shape (features.hip): one wave per 8 x 8 wave tile, lane = pixel.  For each sample of the call, in order:
// the primary ray exactly as the render takes it (block 0 = the jitter, then the thin lens' rounds), Scene::intersect on it once (scene_intersect_wave:
// the grids' wave-cooperative walk, so all 64 lanes stay in the sample loop and in every call, `want` marking the lanes that carry a ray), and the
// hit's object — a miss, or a sample the thin lens yields no ray for, is RMD_ID_MISS — entered into the lane's record by ids_insert.  The record's ten
// words are read once, kept in ten registers and written once: the table is sequential in sample order whatever the rects, so [0, k) + [k, n) is
// [0, n) word for word.  The workgroup is the one-wave-per-item form of the render's launch plan (launch.hpp: plan_render_launch, direct mode).
//
// ids_matte_kernel — one lane per pixel, streaming: the record in, one double out; the sorted keys of the call staged in LDS; the pixels with
// other != 0 counted per wave (a ballot) and added to the call's one counter.
#include "ids_rule.hpp"
#include "render_kernel.hpp"

namespace rmd {

static_assert(kIdWords == RMD_ID_WORDS && kIdSlots == RMD_ID_SLOTS && kIdMiss == RMD_ID_MISS && kIdWords == 2u * kIdSlots + 2u, "ids_rule.hpp mirrors include/raymond_hip.h");

template <bool GRID>
__global__ __launch_bounds__(GRID ? 64 * kGridWavesPerWg : 64) void ids_kernel(RenderParams P, const DevObject *__restrict__ objs, const DevGrid *__restrict__ grids,
                                                                                const WaveTile *__restrict__ tiles, uint32_t wave_lds, uint32_t *__restrict__ ids) {
	extern __shared__ __align__(16) unsigned char smem[];
	DevObject *lobjs = reinterpret_cast<DevObject *>(smem);
	uint32_t *lmasks = reinterpret_cast<uint32_t *>(smem + (size_t)P.n_objects * sizeof(DevObject));
	const uint32_t tid = threadIdx.x, wave = tid >> 6, waves_per_wg = blockDim.x >> 6, lane = tid & 63u;
	{ // stage the object table and the occupancy masks: coalesced, once per workgroup (as features_kernel does; scene_intersect_wave reads them there)
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
	const size_t at = alive ? ((size_t)x + (size_t)y * P.W) * kIdWords : 0;

	uint32_t rec[kIdWords];
#pragma unroll
	for (uint32_t j = 0; j < kIdWords; j++) rec[j] = alive ? ids[at + j] : 0u;

	// the kernel's own loop: sample_count trips, every lane of the wave in it (the walk is wave-cooperative)
	for (uint32_t k = 0; k < P.sample_count; k++) {
		Rng rng;
		rng.init(y * P.W + x, P.sample_begin + k);
		V3 ro, rd;
		double u0, u1;
		rng.next2(P.key0, P.key1, u0, u1); // block 0: the pixel jitter
		primary_ray(P, x, y, u0, u1, ro, rd);
		bool failed = false;
		if (P.use_dof) failed = !thin_lens_from_pinhole(P, ro, rd, rng, ro, rd); // the render's sample is zero there: a miss here
		const bool want = alive && !failed;
		double t = 0.0;
		uint32_t sub = 0;
		const int oi = scene_intersect_wave<GRID>(objs, P.n_objects, grids, lds_masks, scr, want, ro, rd, t, sub, P.axis_pairs, 0u, nullptr, false, P.visit_mask);
		ids_insert(rec, (want && oi >= 0) ? (uint32_t)oi + 1u : kIdMiss); // (a lane that is not alive keeps a record nobody reads)
	}

	if (alive) {
#pragma unroll
		for (uint32_t j = 0; j < kIdWords; j++) ids[at + j] = rec[j];
	}
}

// P.n_work wave tiles; the workgroup's size and LDS are the render's one-wave-per-item plan for this scene (direct mode, no moments)
hipError_t launch_ids(hipStream_t stream, const RenderParams &P, const DevObject *objs, const DevGrid *grids, const WaveTile *wave_tiles, uint32_t *ids) {
	if (P.n_work == 0u || P.sample_count == 0u) return hipSuccess;
	const bool grid = P.n_grids != 0u;
	const LaunchPlan L = plan_render_launch(kModeTiles, grid, P.n_objects, P.mask_words_total, false, false, false, false, P.n_work, 0u);
	if (L.lds > kLdsBudgetBytes || L.waves_per_wg == 0u || L.waves_per_wg > (grid ? kGridWavesPerWg : 1u)) return hipErrorInvalidConfiguration; // (never: check_render_args)
	const void *fn = grid ? reinterpret_cast<const void *>(&ids_kernel<true>) : reinterpret_cast<const void *>(&ids_kernel<false>);
	if (L.lds > 64u * 1024u) {
		hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudgetBytes);
		if (e != hipSuccess) return e;
	}
	const dim3 grid_dim(L.workgroups), block_dim(64u * L.waves_per_wg);
	if (grid) hipLaunchKernelGGL(ids_kernel<true>, grid_dim, block_dim, L.lds, stream, P, objs, grids, wave_tiles, (uint32_t)L.wave_lds, ids);
	else hipLaunchKernelGGL(ids_kernel<false>, grid_dim, block_dim, L.lds, stream, P, objs, grids, wave_tiles, (uint32_t)L.wave_lds, ids);
	return hipGetLastError();
}

constexpr uint32_t kMatteThreads = 256u;

__global__ __launch_bounds__(kMatteThreads) void ids_matte_kernel(const uint32_t *__restrict__ ids, uint64_t n_pixels, const uint32_t *__restrict__ keys, uint32_t n_keys,
                                                                  double *__restrict__ matte, unsigned long long *__restrict__ other_pixels) {
	__shared__ uint32_t lkeys[kIdsMatteMaxObjects];
	for (uint32_t i = threadIdx.x; i < n_keys; i += kMatteThreads) lkeys[i] = keys[i];
	__syncthreads();
	const uint64_t stride = (uint64_t)gridDim.x * kMatteThreads;
	// every lane of a wave makes the same number of trips (the bound is rounded up to the wave), so the ballot sees whole waves
	const uint64_t bound = (n_pixels + 63u) & ~(uint64_t)63u;
	for (uint64_t i = (uint64_t)blockIdx.x * kMatteThreads + threadIdx.x; i < bound; i += stride) {
		const bool inside = i < n_pixels;
		uint32_t rec[kIdWords];
#pragma unroll
		for (uint32_t j = 0; j < kIdWords; j++) rec[j] = inside ? ids[i * kIdWords + j] : 0u;
		if (inside) matte[i] = ids_matte_pixel(rec, lkeys, n_keys);
		const unsigned long long with_other = __ballot(inside && rec[kIdOther] != 0u);
		if ((threadIdx.x & 63u) == 0u && with_other != 0ull) atomicAdd(other_pixels, (unsigned long long)__popcll(with_other));
	}
}

// rmd_ids_matte: matte[i] = ids_matte_pixel of pixel i over the n_keys ascending distinct keys (device memory, at most kIdsMatteMaxObjects), and
// *other_pixels (zeroed by the caller) += the pixels with other != 0
hipError_t launch_ids_matte(hipStream_t stream, const uint32_t *ids, uint64_t n_pixels, const uint32_t *keys, uint32_t n_keys, double *matte, unsigned long long *other_pixels) {
	if (n_pixels == 0u) return hipSuccess;
	if (n_keys > kIdsMatteMaxObjects) return hipErrorInvalidValue; // (never: the caller checks)
	const uint64_t want = (n_pixels + kMatteThreads - 1u) / kMatteThreads;
	const uint32_t blocks = (uint32_t)(want < 65536u ? want : 65536u); // beyond: the kernel's own stride
	hipLaunchKernelGGL(ids_matte_kernel, dim3(blocks), dim3(kMatteThreads), 0, stream, ids, n_pixels, keys, n_keys, matte, other_pixels);
	return hipGetLastError();
}

} // namespace rmd
