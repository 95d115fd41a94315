// First-hit feature buffers (rmd_render_features; include/raymond_hip.h states the definition, DESIGN.md section 12 the structure and its cost).
// A translation unit of its own: the render kernels' code objects do not change.  The kernel's shape is first_hit_body's (first_hit.hpp); its own is
// the sink: the hit's normal / albedo / distance — no hit is seven zeros — added to the lane's 14 running sums in registers, and one
// read-modify-write of the pixel's two 56-byte records per call.
#include "first_hit.hpp"

namespace rmd {

constexpr uint32_t kFeat = RMD_FEATURE_CHANNELS;

struct FeatureSink {
	double *__restrict__ feat, *__restrict__ feat_sq; // (feat_sq may be null)
	double acc[kFeat], sq[kFeat];

	RMD_DEV void load(bool alive, size_t pixel) {
		const size_t rec = alive ? pixel * kFeat : 0;
#pragma unroll
		for (uint32_t j = 0; j < kFeat; j++) acc[j] = alive ? feat[rec + j] : 0.0, sq[j] = (alive && feat_sq) ? feat_sq[rec + j] : 0.0;
	}
	template <bool GRID>
	RMD_DEV void add(bool hit, int oi, const DevObject *lobjs, const DevGrid *__restrict__ grids, const V3 &ro, const V3 &rd, double t, uint32_t sub) {
		double phi[kFeat];
#pragma unroll
		for (uint32_t j = 0; j < kFeat; j++) phi[j] = 0.0;
		if (hit) {
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
	RMD_DEV void store(size_t pixel) {
		const size_t rec = pixel * kFeat;
#pragma unroll
		for (uint32_t j = 0; j < kFeat; j++) feat[rec + j] = acc[j];
		if (feat_sq) {
#pragma unroll
			for (uint32_t j = 0; j < kFeat; j++) feat_sq[rec + j] = sq[j];
		}
	}
};

template <bool GRID>
__global__ __launch_bounds__(GRID ? 64 * kGridWavesPerWg : 64) void features_kernel(RenderParams P, const DevObject *__restrict__ objs,
                                                                                     const DevGrid *__restrict__ grids, const WaveTile *__restrict__ tiles,
                                                                                     uint32_t wave_lds, double *__restrict__ feat, double *__restrict__ feat_sq) {
	FeatureSink sink{feat, feat_sq, {}, {}};
	first_hit_body<GRID>(P, objs, grids, tiles, wave_lds, sink);
}

hipError_t launch_features(hipStream_t stream, const RenderParams &P, const DevObject *objs, const DevGrid *grids, const WaveTile *wave_tiles, double *feat,
                           double *feat_sq) {
	return launch_first_hit(stream, P, &features_kernel<true>, &features_kernel<false>, objs, grids, wave_tiles, feat, feat_sq);
}

} // namespace rmd
