// First-hit object IDs with coverage, and mattes from them (rmd_render_ids, rmd_ids_matte; include/raymond_hip.h states the definition, ids_rule.hpp
// the rule, DESIGN.md section 34 the structure and its cost).  A translation unit of its own: no other unit's code objects change.
//
// ids_kernel<GRID> — first_hit_body's shape (first_hit.hpp); its own is the sink: the hit's object — no hit is RMD_ID_MISS — entered into the
// lane's record by ids_insert.  The record's ten words are read once, kept in ten registers and written once.
//
// ids_matte_kernel — one lane per pixel, streaming: the record in, one double out; the sorted keys of the call staged in LDS; the pixels with
// other != 0 counted per wave (a ballot) and added to the call's one counter.
#include "first_hit.hpp"
#include "ids_rule.hpp"

namespace rmd {

static_assert(kIdWords == RMD_ID_WORDS && kIdSlots == RMD_ID_SLOTS && kIdMiss == RMD_ID_MISS && kIdWords == 2u * kIdSlots + 2u, "ids_rule.hpp mirrors include/raymond_hip.h");

struct IdSink {
	uint32_t *__restrict__ ids;
	uint32_t rec[kIdWords];

	RMD_DEV void load(bool alive, size_t pixel) {
		const size_t at = alive ? pixel * kIdWords : 0;
#pragma unroll
		for (uint32_t j = 0; j < kIdWords; j++) rec[j] = alive ? ids[at + j] : 0u;
	}
	template <bool GRID>
	RMD_DEV void add(bool hit, int oi, const DevObject *, const DevGrid *, const V3 &, const V3 &, double, uint32_t) {
		ids_insert(rec, hit ? (uint32_t)oi + 1u : kIdMiss); // (a lane that is not alive keeps a record nobody reads)
	}
	RMD_DEV void store(size_t pixel) {
#pragma unroll
		for (uint32_t j = 0; j < kIdWords; j++) ids[pixel * kIdWords + j] = rec[j];
	}
};

template <bool GRID>
__global__ __launch_bounds__(GRID ? 64 * kGridWavesPerWg : 64) void ids_kernel(RenderParams P, const DevObject *__restrict__ objs, const DevGrid *__restrict__ grids,
                                                                                const WaveTile *__restrict__ tiles, uint32_t wave_lds, uint32_t *__restrict__ ids) {
	IdSink sink{ids, {}};
	first_hit_body<GRID>(P, objs, grids, tiles, wave_lds, sink);
}

hipError_t launch_ids(hipStream_t stream, const RenderParams &P, const DevObject *objs, const DevGrid *grids, const WaveTile *wave_tiles, uint32_t *ids) {
	return launch_first_hit(stream, P, &ids_kernel<true>, &ids_kernel<false>, objs, grids, wave_tiles, ids);
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
