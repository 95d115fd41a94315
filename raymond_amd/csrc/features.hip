// First-hit feature buffers (rmd_render_features; include/raymond_hip.h states the definition, DESIGN.md section 12 the structure and its cost).
// A translation unit of its own: the render kernels' code objects do not change.
//
// features_kernel<GRID> — one wave per 8 x 8 wave tile, lane = pixel.  For each sample of the call, in order: the primary ray exactly as the render
// takes it (block 0 = the jitter, then the thin lens' rounds), Scene::intersect on it once (scene_intersect_wave, render_kernel.hpp: the grids'
// wave-cooperative walk, so all 64 lanes stay in uniform control flow), and the hit's normal / albedo / distance — a miss, or a sample the thin
// lens yields no ray for, is seven zeros — added to the lane's 14 running sums in registers.  One read-modify-write of the pixel's two 56-byte
// records per call: the sums are sequential in sample order whatever the rects, so [0, k) + [k, n) is [0, n) bit for bit.
// The workgroup is the one-wave-per-item form of the render's launch plan (launch.hpp: plan_render_launch, direct mode): [object table]
// [grid occupancy masks][one area per wave], of which a wave uses the walk scratch.
// f64 throughout, built with -ffp-contract=off like the rest of the library.
#include "render_kernel.hpp"

namespace rmd {

constexpr uint32_t kFeat = RMD_FEATURE_CHANNELS;

template <bool GRID>
__global__ __launch_bounds__(GRID ? 64 * kGridWavesPerWg : 64) void features_kernel(RenderParams P, const DevObject *__restrict__ objs,
                                                                                     const DevGrid *__restrict__ grids, const WaveTile *__restrict__ tiles,
                                                                                     uint32_t wave_lds, double *__restrict__ feat, double *__restrict__ feat_sq) {
	extern __shared__ __align__(16) unsigned char smem[];
	DevObject *lobjs = reinterpret_cast<DevObject *>(smem);
	uint32_t *lmasks = reinterpret_cast<uint32_t *>(smem + (size_t)P.n_objects * sizeof(DevObject));
	const uint32_t tid = threadIdx.x, wave = tid >> 6, waves_per_wg = blockDim.x >> 6, lane = tid & 63u;
	{ // stage the object table and the occupancy masks: coalesced, once per workgroup (as render_kernel_body does)
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
	const size_t rec = alive ? ((size_t)x + (size_t)y * P.W) * kFeat : 0;

	double acc[kFeat], sq[kFeat];
#pragma unroll
	for (uint32_t j = 0; j < kFeat; j++) acc[j] = alive ? feat[rec + j] : 0.0, sq[j] = (alive && feat_sq) ? feat_sq[rec + j] : 0.0;

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
		double phi[kFeat];
#pragma unroll
		for (uint32_t j = 0; j < kFeat; j++) phi[j] = 0.0;
		if (want && oi >= 0) {
			const DevObject &o = lobjs[oi];
			const V3 frag = ro + rd * t; // :246
			V3 normal;
			if (o.geometry_kind == 0u) normal = ld3(o.normal);                        // plane.rs:28-32 (as stored)
			else if (o.geometry_kind == 1u) normal = normalize(frag - ld3(o.origin)); // sphere.rs:31-35
			else if constexpr (GRID) {
				const DevGrid &g = grids[o.grid_index];
				normal = triangle_normal(as_global(g.tri_pos) + (size_t)sub * 9, as_global(g.tri_nrm) + (size_t)sub * 9, as_global(g.tri_aux) + (size_t)sub * 4, frag); // acc_grid.rs:85-87
			} else {
				normal = mk(0.0, 0.0, 0.0); // unreachable: a scene with grid objects runs the GRID instantiation
			}
			phi[0] = normal.x, phi[1] = normal.y, phi[2] = normal.z;
			phi[3] = o.color[0], phi[4] = o.color[1], phi[5] = o.color[2];
			phi[6] = t;
		}
#pragma unroll
		for (uint32_t j = 0; j < kFeat; j++) {
			acc[j] = acc[j] + phi[j];
			sq[j] = sq[j] + phi[j] * phi[j]; // the square rounded, then added (no contraction: -ffp-contract=off)
		}
	}

	if (alive) {
#pragma unroll
		for (uint32_t j = 0; j < kFeat; j++) feat[rec + j] = acc[j];
		if (feat_sq) {
#pragma unroll
			for (uint32_t j = 0; j < kFeat; j++) feat_sq[rec + j] = sq[j];
		}
	}
}

// P.n_work wave tiles; the workgroup's size and LDS are the render's one-wave-per-item plan for this scene (direct mode, no moments)
hipError_t launch_features(hipStream_t stream, const RenderParams &P, const DevObject *objs, const DevGrid *grids, const WaveTile *wave_tiles, double *feat,
                           double *feat_sq) {
	if (P.n_work == 0u || P.sample_count == 0u) return hipSuccess;
	const bool grid = P.n_grids != 0u;
	const LaunchPlan L = plan_render_launch(kModeTiles, grid, P.n_objects, P.mask_words_total, false, false, false, false, P.n_work, 0u);
	if (L.lds > kLdsBudgetBytes || L.waves_per_wg == 0u || L.waves_per_wg > (grid ? kGridWavesPerWg : 1u)) return hipErrorInvalidConfiguration; // (never: check_render_args)
	const void *fn = grid ? reinterpret_cast<const void *>(&features_kernel<true>) : reinterpret_cast<const void *>(&features_kernel<false>);
	if (L.lds > 64u * 1024u) {
		hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudgetBytes);
		if (e != hipSuccess) return e;
	}
	const dim3 grid_dim(L.workgroups), block_dim(64u * L.waves_per_wg);
	if (grid) hipLaunchKernelGGL(features_kernel<true>, grid_dim, block_dim, L.lds, stream, P, objs, grids, wave_tiles, (uint32_t)L.wave_lds, feat, feat_sq);
	else hipLaunchKernelGGL(features_kernel<false>, grid_dim, block_dim, L.lds, stream, P, objs, grids, wave_tiles, (uint32_t)L.wave_lds, feat, feat_sq);
	return hipGetLastError();
}

} // namespace rmd
