// Drives raymond_amd/csrc/resolve_tiles_host.hpp — the host arithmetic of rmd_resolve_tonemap_tiles — through seeded random rect lists on the CPU
// (tests/test_resolve_tiles_host.py builds this with -fsanitize=address,undefined and runs it directly).
//
//   resolve_tiles_table <first list> <lists>
//
// List number s is seeded by s.  Its frame is up to 300 x 200 (every 64th list: one of up to 70000 x 60000, so that a single rect reaches 2^32 - 1
// pixels' neighbourhood) and its rects are drawn from: empty ones (width or height 0), single pixels, rows and columns one pixel wide, tile-sized rects,
// ragged ones, the whole frame, and in the large frames one huge rect.  Checked for every list:
//   * the runs in table order cover the packed pixels 0 .. P - 1 exactly once: the first starts at 0, each starts where the one before it ends, the last
//     ends at P; none is empty, none longer than kResolveRun, none crosses a multiple of kResolveRun (its lanes' groups then number at most 256);
//   * no run spans two rects: [start, start + n) lies inside [first[rect], first[rect + 1]), `local` is start - first[rect], and left, top, width and
//     samples are the rect's;
//   * resolve_locate inverts rect -> packed position: for the first and last pixel of every run, for sampled pixels inside it (all of them in small
//     lists), the (rect, x, y) it returns is the run's rect and the pixel at `local` + offset of that rect, row-major.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "resolve_tiles_host.hpp"

struct Rect {
	uint32_t left, top, width, height;
};

#define REQUIRE(cond, ...)                                          \
	do {                                                            \
		if (!(cond)) {                                              \
			std::fprintf(stderr, "list %" PRIu64 ": ", list);       \
			std::fprintf(stderr, __VA_ARGS__);                      \
			std::fprintf(stderr, " (%s)\n", #cond);                 \
			return false;                                           \
		}                                                           \
	} while (0)

static bool run_list(uint64_t list, uint64_t &runs_seen, uint64_t &located) {
	std::mt19937_64 rng(list);
	auto below = [&](uint64_t n) { return (uint32_t)(rng() % n); };
	const bool large = list % 64 == 63;
	const uint32_t W = large ? 60000u + below(10001) : 1u + below(300), H = large ? 50000u + below(10001) : 1u + below(200);
	std::vector<Rect> rects;
	std::vector<uint32_t> samples;
	uint64_t budget = 0xFFFFFFFFull; // the caller refuses more packed pixels than this
	auto add = [&](Rect r) {
		const uint64_t px = (uint64_t)r.width * r.height;
		if (px > budget) return;
		budget -= px;
		rects.push_back(r), samples.push_back(below(600));
	};
	const uint32_t n_draws = large ? 1u + below(6) : below(40);
	for (uint32_t d = 0; d < n_draws; d++) {
		const uint32_t kind = below(8), x = below(W), y = below(H);
		switch (kind) {
		case 0: add(Rect{x, y, 0u, below(H - y + 1)}); break;                    // no pixels: width 0
		case 1: add(Rect{x, y, below(W - x + 1), 0u}); break;                    // ... height 0
		case 2: add(Rect{x, y, 1u, 1u}); break;                                  // a single pixel
		case 3: add(Rect{0u, y, W, 1u}); break;                                  // a row
		case 4: add(Rect{x, 0u, 1u, H}); break;                                  // a column
		case 5: add(Rect{x, y, std::min(32u, W - x), std::min(32u, H - y)}); break; // a tile, clamped at the edges
		case 6: add(Rect{x, y, 1u + below(W - x), 1u + below(H - y)}); break;    // ragged
		default: add(Rect{0u, 0u, W, H}); break;                                 // the whole frame (in a large one: the huge rect)
		}
	}
	if (large) add(Rect{0u, 0u, W, (uint32_t)std::min<uint64_t>(H, budget / W)}); // one huge rect: what is left of 2^32 - 1 pixels, in whole rows
	const uint32_t n = (uint32_t)rects.size();
	std::vector<uint64_t> first;
	REQUIRE(rmd::resolve_first_pixels(rects.data(), n, W, H, first), "a rect inside the frame was refused");
	REQUIRE(first.size() == (size_t)n + 1 && first[n] <= 0xFFFFFFFFull, "first pixels");
	const std::vector<rmd::ResolveRun> runs = rmd::resolve_runs(rects.data(), samples.data(), n, first);
	uint64_t at = 0;
	for (size_t k = 0; k < runs.size(); k++) {
		const rmd::ResolveRun &r = runs[k];
		REQUIRE(r.start == at, "run %zu starts at %u, the one before it ended at %" PRIu64, k, r.start, at);
		REQUIRE(r.n >= 1 && r.n <= rmd::kResolveRun, "run %zu holds %u pixels", k, r.n);
		REQUIRE(r.start / rmd::kResolveRun == ((uint64_t)r.start + r.n - 1) / rmd::kResolveRun, "run %zu crosses a chunk boundary", k);
		REQUIRE(r.rect < n, "run %zu names rect %u of %u", k, r.rect, n);
		REQUIRE(r.start >= first[r.rect] && (uint64_t)r.start + r.n <= first[r.rect + 1], "run %zu spans two rects", k);
		REQUIRE(r.local == r.start - first[r.rect], "run %zu: local", k);
		const Rect &q = rects[r.rect];
		REQUIRE(r.left == q.left && r.top == q.top && r.width == q.width && r.samples == samples[r.rect], "run %zu does not carry its rect", k);
		const uint32_t stride = large ? 509u : 1u; // (a prime: the samples drift through the rows)
		for (uint32_t o = 0;;) {
			const rmd::ResolvePixel p = rmd::resolve_locate(rects.data(), n, first, (uint64_t)r.start + o);
			const uint64_t local = (uint64_t)r.local + o;
			REQUIRE(p.rect == r.rect && p.x == q.left + local % q.width && p.y == q.top + local / q.width && p.x < q.left + q.width && p.y < q.top + q.height,
			        "packed pixel %" PRIu64 " was located at rect %u (%u, %u)", (uint64_t)r.start + o, p.rect, p.x, p.y);
			located++;
			if (o == r.n - 1) break;
			o = std::min(o + stride, r.n - 1); // (the run's last pixel always)
		}
		at += r.n;
	}
	REQUIRE(at == first[n], "the runs cover %" PRIu64 " of %" PRIu64 " packed pixels", at, first[n]);
	runs_seen += runs.size();
	// a rect that reaches outside the frame is refused
	rects.push_back(Rect{W - 1u, 0u, 2u, 1u});
	REQUIRE(!rmd::resolve_first_pixels(rects.data(), n + 1, W, H, first), "a rect outside the frame was accepted");
	return true;
}

int main(int argc, char **argv) {
	if (argc < 3) return std::fprintf(stderr, "usage: resolve_tiles_table <first list> <lists>\n"), 2;
	const uint64_t begin = std::strtoull(argv[1], nullptr, 10), count = std::strtoull(argv[2], nullptr, 10);
	uint64_t runs = 0, located = 0;
	for (uint64_t list = begin; list < begin + count; list++)
		if (!run_list(list, runs, located)) return 1;
	std::printf("resolve tiles table ok: %" PRIu64 " lists, %" PRIu64 " runs, %" PRIu64 " pixels located\n", count, runs, located);
	return 0;
}
