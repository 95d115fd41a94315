// raymond_amd/csrc/ids_rule.hpp on the CPU, for the host sanitizers (tests/test_ids_host.py builds this with -fsanitize=address,undefined and runs it;
// it is never loaded into Python).  ids_insert and ids_matte_pixel against a second, plain reading of include/raymond_hip.h — a loop over the slots, a
// linear search of the set — on random key sequences; every record, key sequence and key set lives in a heap block of its exact size, so a read or a
// write one word outside is seen.
//   ids_rule_main SEED COUNT
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "ids_rule.hpp"

namespace {
// the header's rule, read again: for j = 0 .. 3 in order, the slot that holds k counts it, the first empty one takes it; else other; then samples
void plain_insert(uint32_t *rec, uint32_t k) {
	bool taken = false;
	for (int j = 0; j < 4 && !taken; j++) {
		if (rec[2 * j] == k) rec[2 * j + 1]++, taken = true;
		else if (rec[2 * j] == 0u) rec[2 * j] = k, rec[2 * j + 1] = 1u, taken = true;
	}
	if (!taken) rec[8]++;
	rec[9]++;
}
double plain_matte(const uint32_t *rec, const uint32_t *objects, size_t n_objects) {
	uint64_t c = 0;
	for (int j = 0; j < 4; j++) {
		bool in = false;
		for (size_t i = 0; i < n_objects; i++) {
			const uint32_t key = objects[i] == 0xFFFFFFFFu ? 0xFFFFFFFFu : objects[i] + 1u;
			if (rec[2 * j] != 0u && rec[2 * j] == key) in = true;
		}
		if (in) c += rec[2 * j + 1];
	}
	return rec[9] == 0u ? 0.0 : (double)c / (double)rec[9];
}
std::unique_ptr<uint32_t[]> block(size_t n) { return std::unique_ptr<uint32_t[]>(new uint32_t[n]); } // exact size: n == 0 is a zero-length block
} // namespace

int main(int argc, char **argv) {
	if (argc < 3) return 2;
	std::mt19937_64 rng((uint64_t)std::strtoull(argv[1], nullptr, 10));
	const long count = std::atol(argv[2]);
	long with_other = 0, full = 0, empty = 0, with_miss = 0, mattes_between = 0, wrapped = 0;
	for (long it = 0; it < count; it++) {
		const size_t n = (size_t)(rng() % 41u);             // 0 .. 40 samples
		const uint32_t pool = 1u + (uint32_t)(rng() % 9u); // 1 .. 9 distinct objects, and the miss
		auto keys = block(n);
		for (size_t i = 0; i < n; i++) {
			const uint32_t o = (uint32_t)(rng() % (pool + 1u));
			keys[i] = o == pool ? rmd::kIdMiss : rmd::ids_key_of(o * 37u); // (object indices 0, 37, 74, ...: key = index + 1)
		}
		auto rec = block(rmd::kIdWords), ref = block(rmd::kIdWords), two = block(rmd::kIdWords);
		std::memset(rec.get(), 0, 40), std::memset(ref.get(), 0, 40), std::memset(two.get(), 0, 40);
		if (it % 16 == 0 && n > 0) { // counts are modulo 2^32: a record that starts one below the wrap in the slot its first key takes
			rec[0] = ref[0] = two[0] = keys[0];
			rec[1] = ref[1] = two[1] = 0xFFFFFFFFu, rec[9] = ref[9] = two[9] = 0xFFFFFFFFu;
			wrapped++;
		}
		const size_t cut = n ? (size_t)(rng() % (n + 1u)) : 0u;
		for (size_t i = 0; i < n; i++) rmd::ids_insert(rec.get(), keys[i]), plain_insert(ref.get(), keys[i]);
		for (size_t i = 0; i < cut; i++) rmd::ids_insert(two.get(), keys[i]); // [0, k) ...
		for (size_t i = cut; i < n; i++) rmd::ids_insert(two.get(), keys[i]); // ... then [k, n), on the words the first left
		if (std::memcmp(rec.get(), ref.get(), 40) || std::memcmp(rec.get(), two.get(), 40)) {
			std::printf("sequence %ld: ids_insert differs from the plain reading\n", it);
			return 1;
		}
		if ((uint32_t)(rec[1] + rec[3] + rec[5] + rec[7] + rec[8]) != rec[9]) {
			std::printf("sequence %ld: the counts do not add up to samples\n", it);
			return 1;
		}
		for (int j = 0; j < 3; j++)
			if (rec[2 * j] == 0u && rec[2 * j + 2] != 0u) {
				std::printf("sequence %ld: an empty slot in front of a used one\n", it);
				return 1;
			}
		with_other += rec[8] != 0u, full += rec[6] != 0u, empty += rec[9] == 0u;
		// the matte: a random set of objects with duplicates; the header's function takes the ascending distinct keys
		const size_t n_obj = (size_t)(rng() % 7u);
		auto objects = block(n_obj);
		for (size_t i = 0; i < n_obj; i++) {
			const uint32_t o = (uint32_t)(rng() % (pool + 2u));
			objects[i] = o >= pool ? (o == pool ? rmd::kIdMiss : 5u) : o * 37u; // (5: an object no sample hit)
			with_miss += objects[i] == rmd::kIdMiss;
		}
		std::vector<uint32_t> sorted;
		for (size_t i = 0; i < n_obj; i++) sorted.push_back(rmd::ids_key_of(objects[i]));
		std::sort(sorted.begin(), sorted.end());
		sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
		auto set = block(sorted.size());
		std::copy(sorted.begin(), sorted.end(), set.get());
		const double got = rmd::ids_matte_pixel(rec.get(), set.get(), (uint32_t)sorted.size()), want = plain_matte(rec.get(), objects.get(), n_obj);
		if (std::memcmp(&got, &want, 8)) {
			std::printf("sequence %ld: ids_matte_pixel %.17g, the plain reading %.17g\n", it, got, want);
			return 1;
		}
		mattes_between += got > 0.0 && got < 1.0;
	}
	std::printf("ids rule ok: %ld sequences, %ld with other, %ld with a full table, %ld without samples, %ld set entries naming the miss, %ld mattes strictly between 0 and 1, %ld near the wrap\n",
	            count, with_other, full, empty, with_miss, mattes_between, wrapped);
	return 0;
}
