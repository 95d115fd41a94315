// Ambient occlusion of the first hit, as exact counts (rmd_render_ao, rmd_ao_resolve; include/raymond_hip.h states the definition, ao_rule.hpp the
// rule, DESIGN.md section 35 the structure and its cost).  A translation unit of its own: no other unit's code objects change.
//
// ao_kernel<GRID> — first_hit_body's shape (first_hit.hpp) with its second segment: the sink keeps the first hit's point and normal, makes the render's
// diffuse bounce ray from them and the sample's next Philox block (trace()'s diffuse branch, src/trace.rs:261-269, through the render kernel's own
// device functions), and counts what Scene::intersect finds on it within max_distance.  The material is not looked at.  The record's four words are
// read once, kept in four registers and written once.
//
// ao_resolve_kernel — ids_matte_kernel's shape: one lane per pixel, streaming: the record in, one double out; the pixels without a first hit counted
// per wave (a ballot) and added to the call's one counter.
#include "first_hit.hpp"
#include "ao_rule.hpp"

namespace rmd {

static_assert(kAoWords == RMD_AO_WORDS, "ao_rule.hpp mirrors include/raymond_hip.h");

struct AoSink {
	static constexpr bool kSecondRay = true;
	uint32_t *__restrict__ ao;
	double max_distance;
	uint32_t rec[kAoWords];
	bool first; // this sample's first hit
	V3 frag, normal;

	RMD_DEV void load(bool alive, size_t pixel) {
		const size_t at = alive ? pixel * kAoWords : 0;
#pragma unroll
		for (uint32_t j = 0; j < kAoWords; j++) rec[j] = alive ? ao[at + j] : 0u;
	}
	template <bool GRID>
	RMD_DEV void add(bool hit, int oi, const DevObject *lobjs, const DevGrid *__restrict__ grids, const V3 &ro, const V3 &rd, double t, uint32_t sub) {
		first = hit;
		// A lane without a first hit builds its follow-up ray from zeros, and onb / normalize may make NaNs of them.  second_ray hands the body `first` as
		// want2: scene_intersect_wave keeps no hit of a lane that is not wanted and counts only wanted lanes where it chooses a path for the wave, and
		// ao_count looks at `occluded` only with a first hit
		frag = mk(0.0, 0.0, 0.0), normal = mk(0.0, 0.0, 0.0);
		if (hit) {
			const DevObject &o = lobjs[oi];
			frag = ro + rd * t; // :246
			// the normal rmd_render_features defines (features.hip)
			if (o.geometry_kind == 0u) normal = ld3(o.normal);                        // plane.rs:28-32 (as stored)
			else if (o.geometry_kind == 1u) normal = normalize(frag - ld3(o.origin)); // sphere.rs:31-35
			else if constexpr (GRID) {
				const DevGrid &g = grids[o.grid_index];
				normal = triangle_normal(as_global(g.tri_pos) + (size_t)sub * 9, as_global(g.tri_nrm) + (size_t)sub * 9, as_global(g.tri_aux) + (size_t)sub * 4, frag); // acc_grid.rs:85-87
			}
		}
	}
	// trace()'s diffuse branch (:261-269, :396-416) with r1, r2 the two 53-bit uniforms of the sample's next block; the block's 22-bit uniform is not used
	RMD_DEV bool second_ray(const RenderParams &P, Rng &rng, V3 &origin, V3 &dir) {
		double r1, r2, pdf;
		rng.next2(P.key0, P.key1, r1, r2);
		V3 local, tg, bt;
		cosine_hemisphere(r1, r2, local, pdf);
		onb(normal, tg, bt);
		dir = normalize(mat3_mul(tg, normal, bt, local)); // :266
		origin = frag + normal * 0.00001;                  // :269
		return first;
	}
	RMD_DEV void second_hit(bool hit2, double t2) {
		ao_count(rec, first, hit2 && t2 < max_distance); // (a NaN distance compares false: open)
	}
	RMD_DEV void store(size_t pixel) {
#pragma unroll
		for (uint32_t j = 0; j < kAoWords; j++) ao[pixel * kAoWords + j] = rec[j];
	}
};

template <bool GRID>
__global__ __launch_bounds__(GRID ? 64 * kGridWavesPerWg : 64) void ao_kernel(RenderParams P, const DevObject *__restrict__ objs, const DevGrid *__restrict__ grids,
                                                                               const WaveTile *__restrict__ tiles, uint32_t wave_lds, uint32_t *__restrict__ ao,
                                                                               double max_distance) {
	AoSink sink{ao, max_distance, {}, false, {}, {}};
	first_hit_body<GRID>(P, objs, grids, tiles, wave_lds, sink);
}

hipError_t launch_ao(hipStream_t stream, const RenderParams &P, const DevObject *objs, const DevGrid *grids, const WaveTile *wave_tiles, uint32_t *ao, double max_distance) {
	return launch_first_hit(stream, P, &ao_kernel<true>, &ao_kernel<false>, objs, grids, wave_tiles, ao, max_distance);
}

constexpr uint32_t kAoResolveThreads = 256u;

__global__ __launch_bounds__(kAoResolveThreads) void ao_resolve_kernel(const uint32_t *__restrict__ ao, uint64_t n_pixels, double empty_value, double *__restrict__ out,
                                                                       unsigned long long *__restrict__ empty_pixels) {
	const uint64_t stride = (uint64_t)gridDim.x * kAoResolveThreads;
	// every lane of a wave makes the same number of trips (the bound is rounded up to the wave), so the ballot sees whole waves
	const uint64_t bound = (n_pixels + 63u) & ~(uint64_t)63u;
	for (uint64_t i = (uint64_t)blockIdx.x * kAoResolveThreads + threadIdx.x; i < bound; i += stride) {
		const bool inside = i < n_pixels;
		uint32_t rec[kAoWords];
#pragma unroll
		for (uint32_t j = 0; j < kAoWords; j++) rec[j] = inside ? ao[i * kAoWords + j] : 0u;
		bool empty = false;
		const double v = ao_resolve_pixel(rec, empty_value, &empty);
		if (inside) out[i] = v;
		const unsigned long long empties = __ballot(inside && empty);
		if ((threadIdx.x & 63u) == 0u && empties != 0ull) atomicAdd(empty_pixels, (unsigned long long)__popcll(empties));
	}
}

// rmd_ao_resolve: out[i] = ao_resolve_pixel of pixel i, and *empty_pixels (zeroed by the caller) += the pixels with open + occluded == 0
hipError_t launch_ao_resolve(hipStream_t stream, const uint32_t *ao, uint64_t n_pixels, double empty_value, double *out, unsigned long long *empty_pixels) {
	if (n_pixels == 0u) return hipSuccess;
	const uint64_t want = (n_pixels + kAoResolveThreads - 1u) / kAoResolveThreads;
	const uint32_t blocks = (uint32_t)(want < 65536u ? want : 65536u); // beyond: the kernel's own stride
	hipLaunchKernelGGL(ao_resolve_kernel, dim3(blocks), dim3(kAoResolveThreads), 0, stream, ao, n_pixels, empty_value, out, empty_pixels);
	return hipGetLastError();
}

} // namespace rmd
