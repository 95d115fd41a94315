// The host mirror's entry points on a machine without a GPU (tests/test_host_no_device.py builds this with raymond.cpp and project.cpp under
// AddressSanitizer and UBSan): every one has to come back with the raymond::Error of rmd_context_create, its owners of device resources destroyed
// on the way out.  It reaches only each function's first failure.
#include <cstdio>
#include <cstring>

#include "raymond.hpp"

using namespace raymond;

static int refused = 0;

template <class F> static void expect_no_device(const char *what, F call) {
	try {
		call();
		std::printf("%s: returned\n", what);
	} catch (const Error &e) {
		const bool named = std::strstr(e.what(), "rmd_context_create") != nullptr;
		std::printf("%s: %s%s\n", what, e.what(), named ? "" : "  (does not name rmd_context_create)");
		refused += named;
	}
}

int main() {
	Settings st;
	st.camera_settings.backbuffer_width = 64, st.camera_settings.backbuffer_height = 64;
	st.sample_count = 4, st.bounce_limit = 2, st.tile_size = {32, 32};
	const Scene scene = reflective_spheres();

	expect_no_device("render_tiled, one worker, one pass", [&] { render_tiled(scene, st).await(); });
	Settings two = st;
	two.samples_per_iteration = 2, two.worker_count = 2;
	expect_no_device("render_tiled, two workers, passes of 2", [&] { render_tiled(scene, two).await(); });
	Settings dual = st;
	dual.samples_per_iteration = 2, dual.denoise = true, dual.denoise_dual = true, dual.adaptive_denoised_threshold = 0.1;
	expect_no_device("render_tiled, dual loop, adaptive", [&] { render_tiled(scene, dual).await(); });

	std::vector<Tile> tiles(1);
	Tile &t = tiles[0];
	t.width = t.height = 2, t.sample_count = 2, t.count_a = t.count_b = 1;
	for (TileData *d : {&t.data, &t.data_sq, &t.data_a, &t.data_sq_a, &t.data_b, &t.data_sq_b}) *d = TileData(4);
	Settings den = st;
	den.denoise = true;
	expect_no_device("denoise_tiles", [&] { denoise_tiles(tiles, den); });
	expect_no_device("denoise_dual_tiles", [&] { denoise_dual_tiles(tiles, den); });
	expect_no_device("render_features", [&] { render_features(scene, st, {rmd_tile_rect{0, 0, 2, 2}}, {1}); });

	std::printf("%d of 6 refused by rmd_context_create\n", refused);
	return refused == 6 ? 0 : 1;
}
