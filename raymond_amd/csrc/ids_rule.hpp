// The rule of the ID buffers (rmd_render_ids, rmd_ids_matte; include/raymond_hip.h states the definition): the lines the kernels (ids.hip), the C++
// mirror (raymond_amd/host) and tests/ids_rule_main.cpp all read.  Needs only <stdint.h>; under hipcc the functions are __host__ __device__.  Integers
// throughout but for the matte's one division.  Written without a loop over the slots and without a dynamically indexed array: in the kernel the ten
// words of a record are ten registers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RMD_IDS_HD __host__ __device__
#else
#define RMD_IDS_HD
#endif

namespace rmd {

constexpr uint32_t kIdSlots = 4u;           // RMD_ID_SLOTS
constexpr uint32_t kIdWords = 10u;          // RMD_ID_WORDS: key_0 count_0 .. key_3 count_3 other samples
constexpr uint32_t kIdOther = 8u, kIdSamples = 9u;
constexpr uint32_t kIdMiss = 0xFFFFFFFFu;   // RMD_ID_MISS
constexpr uint32_t kIdsMatteMaxObjects = 2048u;

// The key of object index o (RMD_ID_MISS stays itself: the background)
RMD_IDS_HD inline uint32_t ids_key_of(uint32_t object) { return object == kIdMiss ? kIdMiss : object + 1u; }

// One sample with key `key`: the first slot in order that holds the key, or is empty, takes it; none: `other`; then `samples`.  Counts wrap at 2^32
RMD_IDS_HD inline void ids_insert(uint32_t rec[kIdWords], uint32_t key) {
	const bool t0 = rec[0] == key || rec[0] == 0u;
	const bool t1 = !t0 && (rec[2] == key || rec[2] == 0u);
	const bool t2 = !t0 && !t1 && (rec[4] == key || rec[4] == 0u);
	const bool t3 = !t0 && !t1 && !t2 && (rec[6] == key || rec[6] == 0u);
	rec[0] = t0 ? key : rec[0], rec[1] += t0 ? 1u : 0u;
	rec[2] = t1 ? key : rec[2], rec[3] += t1 ? 1u : 0u;
	rec[4] = t2 ? key : rec[4], rec[5] += t2 ? 1u : 0u;
	rec[6] = t3 ? key : rec[6], rec[7] += t3 ? 1u : 0u;
	rec[kIdOther] += (t0 || t1 || t2 || t3) ? 0u : 1u;
	rec[kIdSamples] += 1u;
}

// Whether `key` is one of the n ascending, distinct `keys`
RMD_IDS_HD inline bool ids_key_in(const uint32_t *keys, uint32_t n, uint32_t key) {
	uint32_t lo = 0u, hi = n;
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2u;
		if (keys[mid] < key) lo = mid + 1u;
		else hi = mid;
	}
	return lo < n && keys[lo] == key;
}

// The matte of one pixel: the samples of the slots whose key is in the set over the pixel's samples, one division; 0 for a pixel without samples.
// An empty slot (key 0) is in no set, and `other` is never counted
RMD_IDS_HD inline double ids_matte_pixel(const uint32_t rec[kIdWords], const uint32_t *keys, uint32_t n_keys) {
	uint64_t c = 0u;
	if (rec[0] != 0u && ids_key_in(keys, n_keys, rec[0])) c += rec[1];
	if (rec[2] != 0u && ids_key_in(keys, n_keys, rec[2])) c += rec[3];
	if (rec[4] != 0u && ids_key_in(keys, n_keys, rec[4])) c += rec[5];
	if (rec[6] != 0u && ids_key_in(keys, n_keys, rec[6])) c += rec[7];
	const uint32_t samples = rec[kIdSamples];
	return samples == 0u ? 0.0 : (double)c / (double)samples;
}

} // namespace rmd
