// raymond_amd/csrc/ao_rule.hpp on the CPU, for the host sanitizers (tests/test_ao_host.py builds this with -fsanitize=address,undefined and runs it;
// it is never loaded into Python).  ao_count and ao_resolve_pixel against a second, plain reading of include/raymond_hip.h — a branch per outcome, the
// denominator summed in unsigned long long — on random records and outcome sequences; every record lives in a heap block of its exact size, so a read or a write
// one word outside is seen.
//   ao_rule_main SEED COUNT
#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>

#include "ao_rule.hpp"

namespace {
// the header's rule, read again: no first hit is `none`; a first hit is `occluded` or `open`; then `samples`
void plain_count(uint32_t *rec, int outcome) { // 0 none, 1 open, 2 occluded
	if (outcome == 0) rec[2]++;
	else if (outcome == 1) rec[1]++;
	else rec[0]++;
	rec[3]++;
}
// open / (open + occluded): both are below 2^32 and their sum below 2^33, so both conversions are exact and the division rounds once
double plain_resolve(const uint32_t *rec, double empty_value, bool *empty) {
	const unsigned long long open = rec[1], occluded = rec[0];
	*empty = open == 0ull && occluded == 0ull;
	if (*empty) return empty_value;
	const double a = (double)open, b = (double)(open + occluded);
	return a / b;
}
std::unique_ptr<uint32_t[]> block(size_t n) { return std::unique_ptr<uint32_t[]>(new uint32_t[n]); }
} // namespace

int main(int argc, char **argv) {
	if (argc < 3) return 2;
	std::mt19937_64 rng((uint64_t)std::strtoull(argv[1], nullptr, 10));
	const long count = std::atol(argv[2]);
	long wrapped = 0, zero_den = 0, between = 0, all_open = 0, all_occluded = 0, sum_past_32 = 0;
	for (long it = 0; it < count; it++) {
		auto rec = block(rmd::kAoWords), ref = block(rmd::kAoWords), two = block(rmd::kAoWords);
		std::memset(rec.get(), 0, 16), std::memset(ref.get(), 0, 16), std::memset(two.get(), 0, 16);
		const unsigned kind = (unsigned)(rng() % 8u);
		if (kind == 0u) { // counts are modulo 2^32: a record that starts a few below the wrap in every word
			for (uint32_t j = 0; j < 4u; j++) rec[j] = ref[j] = two[j] = 0xFFFFFFFFu - (uint32_t)(rng() % 3u);
			rec[3] = ref[3] = two[3] = (uint32_t)(rec[0] + rec[1] + rec[2]);
			wrapped++;
		} else if (kind == 1u) { // large counts whose sum passes 2^32: the resolve's denominator is a 64-bit sum
			for (uint32_t j = 0; j < 3u; j++) rec[j] = ref[j] = two[j] = 0x80000000u + (uint32_t)(rng() % 0x7FFFFFFFu);
			rec[3] = ref[3] = two[3] = (uint32_t)(rec[0] + rec[1] + rec[2]);
		}
		const size_t n = (size_t)(rng() % 25u); // 0 .. 24 samples
		const unsigned mix = (unsigned)(rng() % 5u); // 0: none only (zero denominators), 1: open only, 2: occluded only, else all three
		auto outcomes = std::unique_ptr<int[]>(new int[n]);
		for (size_t i = 0; i < n; i++) outcomes[i] = mix == 0u ? 0 : mix == 1u ? (int)(rng() % 2u) : mix == 2u ? 2 * (int)(rng() % 2u) : (int)(rng() % 3u);
		const size_t cut = n ? (size_t)(rng() % (n + 1u)) : 0u;
		for (size_t i = 0; i < n; i++) {
			// (ao_count's `occluded` is only looked at with a first hit: a sample without one may carry either value)
			rmd::ao_count(rec.get(), outcomes[i] != 0, outcomes[i] == 2 || (outcomes[i] == 0 && (rng() & 1u)));
			plain_count(ref.get(), outcomes[i]);
		}
		for (size_t i = 0; i < cut; i++) rmd::ao_count(two.get(), outcomes[i] != 0, outcomes[i] == 2); // [0, k) ...
		for (size_t i = cut; i < n; i++) rmd::ao_count(two.get(), outcomes[i] != 0, outcomes[i] == 2); // ... then [k, n), on the words the first left
		if (std::memcmp(rec.get(), ref.get(), 16) || std::memcmp(rec.get(), two.get(), 16)) {
			std::printf("sequence %ld: ao_count differs from the plain reading\n", it);
			return 1;
		}
		if ((uint32_t)(rec[0] + rec[1] + rec[2]) != rec[3]) {
			std::printf("sequence %ld: the counts do not add up to samples\n", it);
			return 1;
		}
		const double empty_value = (rng() & 1u) ? 1.0 : -0.25;
		bool e1 = false, e2 = false;
		const double got = rmd::ao_resolve_pixel(rec.get(), empty_value, &e1), want = plain_resolve(ref.get(), empty_value, &e2);
		if (std::memcmp(&got, &want, 8) || e1 != e2) {
			std::printf("sequence %ld: ao_resolve_pixel %.17g, the plain reading %.17g\n", it, got, want);
			return 1;
		}
		if (!e1 && !(got >= 0.0 && got <= 1.0)) {
			std::printf("sequence %ld: ao_resolve_pixel %.17g outside [0, 1]\n", it, got);
			return 1;
		}
		zero_den += e1, between += !e1 && got > 0.0 && got < 1.0, all_open += !e1 && got == 1.0, all_occluded += !e1 && got == 0.0;
		sum_past_32 += (uint64_t)rec[0] + (uint64_t)rec[1] > 0xFFFFFFFFull;
	}
	std::printf("ao rule ok: %ld records, %ld near the wrap, %ld with a zero denominator, %ld strictly between 0 and 1, %ld all open, %ld all occluded, %ld with open + occluded past 2^32\n",
	            count, wrapped, zero_den, between, all_open, all_occluded, sum_past_32);
	return 0;
}
