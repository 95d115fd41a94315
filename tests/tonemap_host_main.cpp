// Drives raymond_amd/csrc/tonemap_host.hpp — the host's 8-bit output stage for the pixels the tone-map kernels flag — on the CPU
// (tests/test_tonemap_host.py builds this with -fsanitize=address,undefined, runs it directly and holds every pixel to the oracle).
//
//   tonemap_host < records > bytes
//
// A record is six doubles in the machine's byte order: a pixel's three sums, its sample count, the exposure and the gamma.  For each, in order, the
// pixel's three bytes are written.  A trailing partial record is an error.
#include <cstdio>

#include "tonemap_host.hpp"

int main() {
	double rec[6];
	size_t got = 0, records = 0;
	while ((got = std::fread(rec, sizeof(double), 6, stdin)) == 6) {
		uint8_t rgb[3];
		rmd::tonemap_bytes(rec, rec[3], rec[4], 1.0 / rec[5], rgb);
		if (std::fwrite(rgb, 1, 3, stdout) != 3) return std::fprintf(stderr, "tonemap_host: short write\n"), 1;
		records++;
	}
	if (got != 0) return std::fprintf(stderr, "tonemap_host: %zu doubles behind the last whole record\n", got), 2;
	std::fprintf(stderr, "tonemap host ok: %zu records\n", records);
	return std::fflush(stdout) == 0 ? 0 : 1;
}
