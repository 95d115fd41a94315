// raymond_cli — the executable caller of the host mirror; follows cli_old/src/main.rs:35-198
// (build scene -> Settings -> render_tiled -> await -> tone-map -> image file).
//
//   raymond_cli render <spheres|dragon[:n]> W H SPP BOUNCES out.ppm [--raw out.f64] [--gpus N] [--spi K] [--aperture R] [--end-black-paths 1]
//                                                                    [--adaptive THRESHOLD [--adaptive-floor F]]   (needs --spi)
//                                                                    [--adaptive-measure channel_max|luma_tile|luma_pixel]   (what --adaptive compares with
//                                                                      THRESHOLD: rmd_tile_error, or rmd_tile_luma_error's tile_rms or pixel_rms; not with --denoise-dual)
//                                                                    [--adaptive-display T [--adaptive-display-exposure E] [--adaptive-display-gamma G]
//                                                                     [--adaptive-display-floor F] [--adaptive-display-auto-exposure 1]]   (needs --spi; in
//                                                                      place of --adaptive: a tile stops when rmd_tile_weighted_error's rms under
//                                                                      rmd_display_weights' table — its RMS error after exposure and gamma, in fractions of
//                                                                      the display's full scale — is at most T; not with --denoise-dual)
//                                                                    [--dump-tiles FILE]   (one "left top width height sample_count error" line per finished tile)
//                                                                    [--tile-size N]   (N x N tiles instead of 32 x 32)
//                                                                    [--denoise 1 [--denoise-radius R] [--denoise-patch F] [--denoise-k K]
//                                                                     [--denoise-alpha A]]   (the image is rmd_denoise's, on GPU 0)
//                                                                    [--denoise-features 1 [--denoise-feature-k K] [--denoise-feature-tau T]]
//                                                                      (needs --denoise 1: first-hit features guide the filter, rmd_denoise_guided)
//                                                                    [--denoise-feature-slope G]   (needs a guided non-local-means filter — --denoise-features,
//                                                                      --denoise-dual-features or --denoise-dual-select —, not with the a-trous ones: the
//                                                                      feature-slope term at G pixels, the _slope calls; 3 is the value to start from)
//                                                                    [--denoise-atrous 1 [--denoise-atrous-levels N] [--denoise-atrous-k K]]
//                                                                      (needs --denoise 1, not with --denoise-dual: the fast filter for previews,
//                                                                       rmd_denoise_atrous, guided with --denoise-features 1)
//                                                                    [--denoise-atrous-slope G]   (needs a guided a-trous filter — --denoise-atrous 1 with --denoise-features 1,
//                                                                      or --denoise-dual-atrous 1 with --denoise-dual-features 1: the feature-slope term at G
//                                                                      pixels in rmd_denoise_atrous_slope / rmd_denoise_atrous_dual_slope[_region]; 3 to start from)
//                                                                    [--dump-features FILE]   (the W*H*7 feature means as raw f64: the AOVs)
//                                                                    [--dump-ids FILE]   (the W*H*10 first-hit ID words as raw little-endian uint32, rmd_render_ids over
//                                                                      the finished tiles at their own counts: key_0 count_0 .. key_3 count_3 other samples)
//                                                                    [--dump-matte FILE --matte-objects 0,3,miss]   (rmd_ids_matte of those words for the listed
//                                                                      object indices, `miss` the background, as raw f64; prints the pixels whose table overflowed)
//                                                                    [--dump-ao FILE --ao-distance D [--ao-empty V]]   (rmd_render_ao over the finished tiles at their own
//                                                                      counts, the bounce ray off the first hit occluded by a hit nearer than D — inf: any hit —, and
//                                                                      rmd_ao_resolve of it as raw f64: open / (open + occluded), V, by default 1, where no sample has
//                                                                      a first hit; prints the number of such pixels)
//                                                                    [--denoise-dual 1 [--adaptive-denoised T [--adaptive-min N]]]
//                                                                      (needs --denoise 1 and --spi, one GPU: passes alternate between two half buffers,
//                                                                       the image is rmd_denoise_dual's; T: tiles finish by rmd_tile_error_dual)
//                                                                    [--adaptive-denoised-display T]   (needs --denoise-dual 1 and --spi, in place of
//                                                                      --adaptive-denoised: tiles finish when rmd_tile_weighted_error_dual's rms — the filtered
//                                                                      frame's error after exposure and gamma, under rmd_display_weights' table at the
//                                                                      --adaptive-display-exposure / -gamma / -floor / -auto-exposure options — is at most T)
//                                                                    [--denoise-dual-features 1]   (needs --denoise-dual 1: first-hit features guide the dual
//                                                                      filter, rmd_denoise_dual_guided, with --denoise-feature-k / --denoise-feature-tau)
//                                                                    [--denoise-dual-select 1]     (needs --denoise-dual 1: per pixel the better of the unguided
//                                                                      filter at --denoise-k and the guided one at k = 1, rmd_denoise_dual_select)
//                                                                    [--denoise-dual-atrous 1]     (needs --denoise-dual 1, not with --denoise-dual-select: the fast filter
//                                                                      on the two halves, rmd_denoise_atrous_dual, at --denoise-atrous-levels / --denoise-atrous-k,
//                                                                      guided with --denoise-dual-features 1; the adaptive check calls it on the whole frame)
//                                                                    [--denoise-dual-atrous-region 1] (needs --denoise-dual-atrous 1: the adaptive check calls
//                                                                      rmd_denoise_atrous_dual_region over the live tiles instead; the same output)
//                                                                    [--preview-every N --preview-prefix PATH [--preview-denoise 1] [--preview-exposure E]
//                                                                     [--preview-gamma G]]   (needs --spi, one GPU: after every N-th pass that leaves the
//                                                                      render unfinished the frame so far, tone-mapped on the GPU, is written to
//                                                                      PATH_0001.ppm, PATH_0002.ppm, ...; --preview-denoise 1: the fast filter's frame)
//                                                                    [--progress-tiles 0]   (no TileProgressed snapshot is made or downloaded)
//                                                                    [--auto-exposure 1 [--auto-exposure-percentile P] [--auto-exposure-target T]]
//                                                                      (the exposure that puts the P-th part of the luminance histogram, 0.99, at T, 0.8,
//                                                                       before gamma — rmd_exposure_from_histogram —: for every preview from
//                                                                       rmd_luminance_histogram_tiles on what it resolves, in place of --preview-exposure, and
//                                                                       for out.ppm from the final frame's histogram, made on the host; --raw is untouched)
//                                                                    [--despike 1 [--despike-radius R] [--despike-rank N] [--despike-k K] [--despike-ratio Q]
//                                                                     [--despike-floor F]]   (firefly rejection, rmd_despike at 2, 2, 6, 2, 0, in front of
//                                                                      the plain divide or of whichever --denoise filter is on, and of the --adaptive check;
//                                                                      not with --denoise-dual)
//                                                                    [--despike-dual 1]   (with --denoise-dual: rmd_despike_dual at the --despike-* values in front
//                                                                      of the dual filter, in await() and in every filter call of the dual loop)
//   raymond_cli mesh N out.bin            procedural stand-in mesh as raw f64 (tri_pos then tri_nrm)
//   raymond_cli ply in.ply out.bin        Mesh::load_ply + bake_transform(0,-0.3,2.9), raw f64 as above
//   raymond_cli tiles W H TW TH           tile generation order of render_tiled, one "left top width height" per line
//   raymond_cli project in.json dump|json Project::load (core/src/project.rs): flattened scene, or the re-serialised JSON
//   raymond_cli tilemsg W H               a TileFinished message in the wire form of server/src/protocol.rs
//   raymond_cli lumahist in.f64 [P T]     the luminance histogram of a --raw frame, made on the host (raymond::luminance_histogram): one line of its 262
//                                         counters in rmd_luma_histogram's order, one with rmd_exposure_from_histogram's exposure at P (0.99) and T (0.8)
//   raymond_cli despike S.f64 Q.f64 W H rects.txt R N K Q F outS.f64 outQ.f64
//                                         rmd_despike made on the host (raymond::despike_host, from the header the kernel is built from) over raw W*H*3 f64
//                                         sums and sums of squares; rects.txt: one "left top width height count" per line; K, Q and F are read as C99
//                                         hexadecimal or decimal doubles; prints one line of the spikes per rect
//   raymond_cli despike-dual SA.f64 QA.f64 SB.f64 QB.f64 W H rects.txt R N K Q F outSA.f64 outQA.f64 outSB.f64 outQB.f64
//                                         rmd_despike_dual made on the host (raymond::despike_dual_host) over the two halves' raw W*H*3 f64 sums and sums of
//                                         squares; rects.txt: one "left top width height count_a count_b" per line; the rest as for despike
//   raymond_cli tile-luma-error S.f64 Q.f64 W H rects.txt FLOOR
//                                         rmd_tile_luma_error made on the host (raymond::tile_luma_error_host, from the header the kernel is built from) over raw
//                                         W*H*3 f64 sums and sums of squares; rects.txt as for despike; FLOOR is read as a C99 hexadecimal or decimal double;
//                                         prints per rect "tile_rms pixel_rms mean_luma mean_variance mean_rel_variance valid invalid", doubles as %.17g
//   raymond_cli tile-weighted-error S.f64 Q.f64 W H rects.txt EXPOSURE GAMMA FLOOR | S.f64 Q.f64 W H rects.txt --weights weights.f64
//                                         rmd_tile_weighted_error made on the host (raymond::tile_weighted_error_host, from the header the kernel is built from)
//                                         over raw W*H*3 f64 sums and sums of squares, under rmd_display_weights' table at EXPOSURE, GAMMA and FLOOR (C99
//                                         hexadecimal or decimal doubles) or under the 260 raw f64 weights of weights.f64; rects.txt as for despike; prints per
//                                         rect "rms mean_weighted_variance mean_luma mean_variance valid invalid", doubles as their 64 bits in hexadecimal
//   raymond_cli tile-weighted-error-dual OUT.f64 ERR.f64 W H rects.txt EXPOSURE GAMMA FLOOR | OUT.f64 ERR.f64 W H rects.txt --weights weights.f64
//                                         rmd_tile_weighted_error_dual made on the host (raymond::tile_weighted_error_dual_host, from the header the kernel is
//                                         built from) over the raw W*H*3 f64 filtered means OUT and the W*H f64 error image ERR, under the table as above;
//                                         rects.txt as for despike, its count column read and ignored; prints per rect
//                                         "rms mean_weighted_variance mean_luma mean_variance valid invalid", doubles as their 64 bits in hexadecimal
//   raymond_cli ids-matte IDS.u32 W H LIST OUT.f64
//                                         rmd_ids_matte made on the host (raymond::ids_matte_host, from the header the kernel is built from; no GPU) over raw
//                                         W*H*10 uint32 ID words; LIST: object indices and `miss`, comma-separated, or `none`; prints the pixels with other != 0
//   raymond_cli ao-resolve AO.u32 W H OUT.f64 [EMPTY]
//                                         rmd_ao_resolve made on the host (raymond::ao_resolve_host, from the header the kernel is built from; no GPU) over raw
//                                         W*H*4 uint32 AO words; EMPTY: the value of a pixel without a first hit, by default 1; prints the number of such pixels
//   raymond_cli intersect SCENE --rays IN.f64 --out OUT.hits
//                                         rmd_intersect_rays (raymond::intersect_rays, GPU 0) on the rays of IN.f64: raw f64, 6 a ray — origin xyz, direction xyz,
//                                         the direction used as given; a file whose size is no multiple of 48 bytes is refused.  OUT.hits: one raw 40-byte
//                                         rmd_ray_hit a ray (t, normal xyz as f64, object as int32, triangle as uint32; a miss is 0, zeros, -1, 0).  SCENE:
//                                         spheres, dragon[:n], project:in.json, or the path of a project file.  Prints the number of rays and of hits
//   raymond_cli pick SCENE --pixel X,Y [--size W,H] [--fov DEGREES] [--position X,Y,Z]
//                                         what pixel (X, Y) of a W x H frame (by default 1920,1080) sees through its centre, from a camera of vertical field of view
//                                         DEGREES (55) at X,Y,Z (0,0,0): rmd_camera_rays and rmd_intersect_rays on GPU 0 (raymond::pick).  Prints ONE line,
//                                         "object triangle t nx ny nz": the object's index in the scene (-1: the background) and the mesh triangle (0 for a plane,
//                                         a sphere and the background) as decimal integers, the distance and the normal as %.17g doubles.  A pixel outside the
//                                         frame, a malformed option or one without its value is refused before the scene is built
//   raymond_cli display-weights EXPOSURE GAMMA FLOOR
//                                         rmd_display_weights: its 260 weights, one per line, as their 64 bits in hexadecimal
//   raymond_cli hostapi <spheres|dragon[:n]> W H SPP BOUNCES SPI [--end-black-paths 1] [--preview-every N [--preview-denoise 1]] [--progress-tiles 0]
//                                         what a drop-in caller gets: one JSON line with the wall time of render_tiled -> last TileFinished
//   (render also accepts `project:in.json` as its scene)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <thread>

#include "raymond.hpp"

using namespace raymond;

// A consumer of a progressive render: every message through poll() (src/trace.rs:115-117) as it arrives — TileProgressed snapshots are counted,
// TileFinished tiles are assembled into the image as await() would (:93-99).  (await() itself stops collecting at the first message that is not
// TileFinished, :101-103: with snapshots of several workers in the channel it is only safe once they have been drained.)  With st.denoise the
// finished tiles go through denoise_tiles on GPU 0 once the workers have left, as await() would.  FramePreview messages are written as
// <preview_prefix>_0001.ppm, _0002.ppm, ... in the order they arrive (dropped without a prefix).
static std::vector<Vector3> consume(TaskHandle &handle, const Settings &st, size_t &progressed, double *last_finished_s = nullptr,
                                    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), const Scene *scene = nullptr,
                                    std::vector<double> *feature_means = nullptr, std::vector<Tile> *finished_out = nullptr, const std::string &preview_prefix = "",
                                    size_t *previews_out = nullptr) {
	const size_t W = st.camera_settings.backbuffer_width, H = st.camera_settings.backbuffer_height;
	const size_t n_tiles = generate_tiles(W, H, st.tile_size).size();
	std::vector<Tile> finished_tiles; // (zero-copy views of the download's block: taking them is cheap; the image is assembled afterwards)
	finished_tiles.reserve(n_tiles);
	size_t previews = 0;
	for (;;) {
		const bool done = handle.finished(); // read BEFORE the channel is drained: nothing is sent after the last worker has left
		while (std::optional<Message> m = handle.poll()) {
			if (m->kind == Message::TileProgressed) {
				progressed++;
				continue;
			}
			if (m->kind == Message::FramePreview) {
				char number[32];
				std::snprintf(number, sizeof(number), "_%04zu.ppm", ++previews);
				if (!preview_prefix.empty()) write_ppm(preview_prefix + number, m->preview->rgb8, m->preview->width, m->preview->height);
				continue;
			}
			finished_tiles.push_back(std::move(m->tile));
			if (finished_tiles.size() == n_tiles && last_finished_s) *last_finished_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		}
		if (done || finished_tiles.size() == n_tiles) break;
		std::this_thread::sleep_for(std::chrono::microseconds(100));
	}
	if (previews_out) *previews_out = previews;
	if (st.denoise) {
		handle.await(); // (its channel is drained: it only waits for the workers and rethrows a worker's error)
		std::vector<Vector3> den = finished_tiles.empty() ? std::vector<Vector3>(W * H, Vector3{0, 0, 0})
		                           : st.denoise_dual      ? denoise_dual_tiles(finished_tiles, st, 0, nullptr, scene)
		                                                  : denoise_tiles(finished_tiles, st, 0, scene, feature_means);
		if (finished_out) *finished_out = std::move(finished_tiles);
		return den;
	}
	if (finished_out) *finished_out = finished_tiles; // (views: cheap)
	if (st.despike && !finished_tiles.empty()) { // await()'s plain path with the setting on: the divide of the despiked sums
		handle.await();
		return despike_tiles(finished_tiles, st, 0);
	}
	std::vector<Vector3> image(W * H, Vector3{0, 0, 0});
	for (const Tile &t : finished_tiles) place_tile(t, t.data, W, image, (double)t.sample_count); // :95
	handle.await(); // waits for the workers to leave (they free their device memory after their last message); rethrows a worker's error
	return image;
}

// "0,3,miss" -> object indices, `miss` = RMD_ID_MISS; "none" or "" = the empty set
static std::vector<uint32_t> parse_objects(const std::string &list) {
	std::vector<uint32_t> out;
	if (list == "none") return out;
	for (size_t at = 0; at < list.size();) {
		const size_t end = std::min(list.find(',', at), list.size());
		const std::string word = list.substr(at, end - at);
		if (word == "miss") out.push_back(RMD_ID_MISS);
		else if (!word.empty() && word.find_first_not_of("0123456789") == std::string::npos) out.push_back((uint32_t)std::strtoul(word.c_str(), nullptr, 10));
		else throw Error(RMD_ERR_INVALID_ARGUMENT, "object list: an index or `miss`, not '" + word + "'");
		at = end + 1;
	}
	return out;
}

// spheres | dragon[:n] | project:in.json | in.json (render's scene words, and a bare project path)
static Scene scene_of(const std::string &what) {
	if (what == "spheres") return reflective_spheres();
	if (what.rfind("dragon", 0) == 0) return gold_dragon_standin(what.size() > 7 ? std::atoi(what.c_str() + 7) : 91);
	if (what.rfind("project:", 0) == 0) return Project::load(what.substr(8)).build_scene(); // core/src/project.rs
	if (what.size() > 5 && what.compare(what.size() - 5, 5, ".json") == 0) return Project::load(what).build_scene();
	throw Error(RMD_ERR_INVALID_ARGUMENT, "unknown scene " + what);
}

// "a,b[,c]" -> exactly n numbers, each read whole by `read`; anything else is refused under the option's name
template <class T, class Read>
static std::vector<T> parse_list(const char *option, const std::string &text, size_t n, Read read) {
	std::vector<T> out;
	for (size_t at = 0; at <= text.size();) {
		const size_t end = std::min(text.find(',', at), text.size());
		const std::string word = text.substr(at, end - at);
		char *stop = nullptr;
		const T v = read(word.c_str(), &stop);
		if (word.empty() || word[0] == ' ' || *stop != '\0') throw Error(RMD_ERR_INVALID_ARGUMENT, std::string(option) + ": not a number: '" + word + "'");
		out.push_back(v);
		at = end + 1;
	}
	if (out.size() != n) throw Error(RMD_ERR_INVALID_ARGUMENT, std::string(option) + ": " + std::to_string(n) + " comma-separated values, not '" + text + "'");
	return out;
}
static std::vector<uint32_t> parse_u32s(const char *option, const std::string &text, size_t n) {
	return parse_list<uint32_t>(option, text, n, [&](const char *w, char **stop) -> uint32_t {
		if (*w < '0' || *w > '9') throw Error(RMD_ERR_INVALID_ARGUMENT, std::string(option) + ": not an unsigned integer: '" + w + "'");
		const unsigned long long v = std::strtoull(w, stop, 10);
		if (v > 0xFFFFFFFFull) throw Error(RMD_ERR_INVALID_ARGUMENT, std::string(option) + ": above 2^32 - 1: '" + w + "'");
		return (uint32_t)v;
	});
}
static std::vector<double> parse_doubles(const char *option, const std::string &text, size_t n) {
	return parse_list<double>(option, text, n, [](const char *w, char **stop) { return std::strtod(w, stop); });
}

static void dump_mesh(const Mesh &m, const std::string &path) {
	std::ofstream f(path, std::ios::binary);
	f.write(reinterpret_cast<const char *>(m.tri_pos.data()), (std::streamsize)(m.tri_pos.size() * 8));
	f.write(reinterpret_cast<const char *>(m.tri_nrm.data()), (std::streamsize)(m.tri_nrm.size() * 8));
}

int main(int argc, char **argv) {
	try {
		if (argc >= 4 && !std::strcmp(argv[1], "mesh")) {
			dump_mesh(lumpy_sphere_mesh(std::atoi(argv[2])), argv[3]);
			return 0;
		}
		if (argc >= 4 && !std::strcmp(argv[1], "ply")) {
			Mesh m = Mesh::load_ply(argv[2]);
			m.bake_transform({0.0, -0.3, 2.9});
			dump_mesh(m, argv[3]);
			std::printf("%zu triangles\n", m.triangle_count());
			return 0;
		}
		if (argc >= 4 && !std::strcmp(argv[1], "project")) {
			Project p = Project::load(argv[2]);
			if (!std::strcmp(argv[3], "json")) {
				std::printf("%s\n", p.dumps().c_str());
				return 0;
			}
			Scene sc = p.build_scene();
			for (const Object &o : sc.objects) {
				const Geometry &g = o.geometry;
				if (g.kind == RMD_GEOM_PLANE) std::printf("plane %.17g %.17g %.17g %.17g %.17g %.17g", g.plane.origin[0], g.plane.origin[1], g.plane.origin[2], g.plane.normal[0], g.plane.normal[1], g.plane.normal[2]);
				else if (g.kind == RMD_GEOM_SPHERE) std::printf("sphere %.17g %.17g %.17g %.17g", g.sphere.origin[0], g.sphere.origin[1], g.sphere.origin[2], g.sphere.radius);
				else {
					const rmd_grid_desc &d = g.grid->desc();
					unsigned long long h = 1469598103934665603ull; // FNV-1a over cells then mapping_table
					for (uint64_t i = 0; i < d.n_cells; i++) h = (h ^ d.cells[i]) * 1099511628211ull;
					for (uint64_t i = 0; i < d.n_mapping; i++) h = (h ^ d.mapping_table[i]) * 1099511628211ull;
					std::printf("grid %u %u %u %llu %llu %llu", d.resolution[0], d.resolution[1], d.resolution[2], (unsigned long long)d.n_tris, (unsigned long long)d.n_mapping, h);
				}
				const Material &m = o.material;
				std::printf(" | %u %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", m.kind, m.color[0], m.color[1], m.color[2], m.roughness, m.aux[0], m.aux[1], m.aux[2], m.aux[3], m.aux[4]);
			}
			return 0;
		}
		if (argc >= 4 && !std::strcmp(argv[1], "tilemsg")) {
			Message msg;
			msg.kind = Message::TileFinished;
			msg.tile.width = std::atoi(argv[2]), msg.tile.height = std::atoi(argv[3]), msg.tile.left = 32, msg.tile.top = 64, msg.tile.sample_count = 7;
			for (size_t i = 0; i < msg.tile.width * msg.tile.height; i++) msg.tile.data.push_back({0.125 * (double)i, 1.0 / (double)(i + 3), -2.5e-7 * (double)i});
			std::printf("%s\n", message_to_json(msg).c_str());
			return 0;
		}
		if (argc >= 3 && !std::strcmp(argv[1], "lumahist")) {
			std::ifstream f(argv[2], std::ios::binary | std::ios::ate);
			if (!f) throw Error(RMD_ERR_INVALID_ARGUMENT, std::string("cannot read ") + argv[2]);
			std::vector<Vector3> image((size_t)f.tellg() / sizeof(Vector3));
			f.seekg(0);
			f.read(reinterpret_cast<char *>(image.data()), (std::streamsize)(image.size() * sizeof(Vector3)));
			const rmd_luma_histogram h = luminance_histogram(image);
			for (uint32_t i = 0; i < RMD_LUMA_BINS; i++) std::printf("%llu ", (unsigned long long)h.bins[i]);
			std::printf("%llu %llu %llu %llu %llu %llu\n", (unsigned long long)h.below, (unsigned long long)h.above, (unsigned long long)h.zero,
			            (unsigned long long)h.negative, (unsigned long long)h.not_finite, (unsigned long long)h.pixels);
			double exposure = 0.0;
			if (rmd_exposure_from_histogram(&h, argc > 3 ? std::atof(argv[3]) : 0.99, argc > 4 ? std::atof(argv[4]) : 0.8, &exposure) != RMD_OK)
				throw Error(RMD_ERR_INVALID_ARGUMENT, rmd_last_error(nullptr));
			std::printf("%.17g\n", exposure);
			return 0;
		}
		if (argc >= 14 && !std::strcmp(argv[1], "despike")) {
			const size_t W = (size_t)std::atoll(argv[4]), H = (size_t)std::atoll(argv[5]);
			std::vector<Vector3> sums(W * H), sums_sq(W * H), out, out_sq;
			for (int i = 0; i < 2; i++) {
				std::ifstream f(argv[2 + i], std::ios::binary);
				std::vector<Vector3> &dst = i ? sums_sq : sums;
				if (!f || !f.read(reinterpret_cast<char *>(dst.data()), (std::streamsize)(dst.size() * sizeof(Vector3))))
					throw Error(RMD_ERR_INVALID_ARGUMENT, std::string("cannot read ") + argv[2 + i]);
			}
			std::vector<rmd_tile_rect> rects;
			std::vector<uint32_t> counts;
			std::ifstream rf(argv[6]);
			for (rmd_tile_rect r; rf >> r.left >> r.top >> r.width >> r.height;) {
				uint32_t n = 0;
				rf >> n;
				rects.push_back(r), counts.push_back(n);
			}
			const std::vector<uint32_t> replaced = despike_host(sums, sums_sq, W, H, rects, counts, (uint32_t)std::atoi(argv[7]), (uint32_t)std::atoi(argv[8]), std::strtod(argv[9], nullptr),
			                                                    std::strtod(argv[10], nullptr), std::strtod(argv[11], nullptr), out, out_sq);
			for (int i = 0; i < 2; i++) {
				std::ofstream f(argv[12 + i], std::ios::binary);
				const std::vector<Vector3> &src = i ? out_sq : out;
				f.write(reinterpret_cast<const char *>(src.data()), (std::streamsize)(src.size() * sizeof(Vector3)));
			}
			for (uint32_t n : replaced) std::printf("%u ", n);
			std::printf("\n");
			return 0;
		}
		if (argc >= 18 && !std::strcmp(argv[1], "despike-dual")) {
			const size_t W = (size_t)std::atoll(argv[6]), H = (size_t)std::atoll(argv[7]);
			std::vector<Vector3> in[4], out[4]; // SA, QA, SB, QB
			for (int i = 0; i < 4; i++) {
				in[i].resize(W * H);
				std::ifstream f(argv[2 + i], std::ios::binary);
				if (!f || !f.read(reinterpret_cast<char *>(in[i].data()), (std::streamsize)(in[i].size() * sizeof(Vector3))))
					throw Error(RMD_ERR_INVALID_ARGUMENT, std::string("cannot read ") + argv[2 + i]);
			}
			std::vector<rmd_tile_rect> rects;
			std::vector<uint32_t> counts_a, counts_b;
			std::ifstream rf(argv[8]);
			for (rmd_tile_rect r; rf >> r.left >> r.top >> r.width >> r.height;) {
				uint32_t na = 0, nb = 0;
				rf >> na >> nb;
				rects.push_back(r), counts_a.push_back(na), counts_b.push_back(nb);
			}
			const std::vector<uint32_t> replaced =
			    despike_dual_host(in[0], in[1], in[2], in[3], W, H, rects, counts_a, counts_b, (uint32_t)std::atoi(argv[9]), (uint32_t)std::atoi(argv[10]), std::strtod(argv[11], nullptr),
			                      std::strtod(argv[12], nullptr), std::strtod(argv[13], nullptr), out[0], out[1], out[2], out[3]);
			for (int i = 0; i < 4; i++) {
				std::ofstream f(argv[14 + i], std::ios::binary);
				f.write(reinterpret_cast<const char *>(out[i].data()), (std::streamsize)(out[i].size() * sizeof(Vector3)));
			}
			for (uint32_t n : replaced) std::printf("%u ", n);
			std::printf("\n");
			return 0;
		}
		if (argc >= 8 && !std::strcmp(argv[1], "tile-luma-error")) {
			const size_t W = (size_t)std::atoll(argv[4]), H = (size_t)std::atoll(argv[5]);
			std::vector<Vector3> sums(W * H), sums_sq(W * H);
			for (int i = 0; i < 2; i++) {
				std::ifstream f(argv[2 + i], std::ios::binary);
				std::vector<Vector3> &dst = i ? sums_sq : sums;
				if (!f || !f.read(reinterpret_cast<char *>(dst.data()), (std::streamsize)(dst.size() * sizeof(Vector3))))
					throw Error(RMD_ERR_INVALID_ARGUMENT, std::string("cannot read ") + argv[2 + i]);
			}
			std::vector<rmd_tile_rect> rects;
			std::vector<uint32_t> counts;
			std::ifstream rf(argv[6]);
			for (rmd_tile_rect r; rf >> r.left >> r.top >> r.width >> r.height;) {
				uint32_t n = 0;
				rf >> n;
				rects.push_back(r), counts.push_back(n);
			}
			for (const rmd_tile_luma &t : tile_luma_error_host(sums, sums_sq, W, H, rects, counts, std::strtod(argv[7], nullptr)))
				std::printf("%.17g %.17g %.17g %.17g %.17g %u %u\n", t.tile_rms, t.pixel_rms, t.mean_luma, t.mean_variance, t.mean_rel_variance, t.valid, t.invalid);
			return 0;
		}
		if (argc >= 7 && !std::strcmp(argv[1], "ids-matte")) {
			const size_t W = (size_t)std::atoll(argv[3]), H = (size_t)std::atoll(argv[4]);
			std::vector<uint32_t> words(W * H * RMD_ID_WORDS);
			std::ifstream f(argv[2], std::ios::binary);
			if (!f || (!words.empty() && !f.read(reinterpret_cast<char *>(words.data()), (std::streamsize)(words.size() * sizeof(uint32_t)))))
				throw Error(RMD_ERR_INVALID_ARGUMENT, std::string("cannot read ") + argv[2]);
			uint64_t other = 0;
			const std::vector<double> matte = ids_matte_host(words, W, H, parse_objects(argv[5]), &other);
			std::ofstream o(argv[6], std::ios::binary);
			o.write(reinterpret_cast<const char *>(matte.data()), (std::streamsize)(matte.size() * 8));
			std::printf("%llu\n", (unsigned long long)other);
			return 0;
		}
		if (argc >= 6 && !std::strcmp(argv[1], "ao-resolve")) {
			const size_t W = (size_t)std::atoll(argv[3]), H = (size_t)std::atoll(argv[4]);
			std::vector<uint32_t> words(W * H * RMD_AO_WORDS);
			std::ifstream f(argv[2], std::ios::binary);
			if (!f || (!words.empty() && !f.read(reinterpret_cast<char *>(words.data()), (std::streamsize)(words.size() * sizeof(uint32_t)))))
				throw Error(RMD_ERR_INVALID_ARGUMENT, std::string("cannot read ") + argv[2]);
			uint64_t empty = 0;
			const std::vector<double> out = ao_resolve_host(words, W, H, argc >= 7 ? std::strtod(argv[6], nullptr) : 1.0, &empty);
			std::ofstream o(argv[5], std::ios::binary);
			o.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)(out.size() * 8));
			std::printf("%llu\n", (unsigned long long)empty);
			return 0;
		}
		if (argc >= 2 && !std::strcmp(argv[1], "intersect")) {
			std::string rays_path, out_path;
			if (argc < 3 || (argc - 3) % 2 != 0) throw Error(RMD_ERR_INVALID_ARGUMENT, "intersect: SCENE --rays IN.f64 --out OUT.hits");
			for (int i = 3; i + 1 < argc; i += 2) {
				if (!std::strcmp(argv[i], "--rays")) rays_path = argv[i + 1];
				else if (!std::strcmp(argv[i], "--out")) out_path = argv[i + 1];
				else throw Error(RMD_ERR_INVALID_ARGUMENT, std::string("intersect: unknown option ") + argv[i]);
			}
			if (rays_path.empty() || out_path.empty()) throw Error(RMD_ERR_INVALID_ARGUMENT, "intersect: --rays and --out are both needed");
			std::ifstream f(rays_path, std::ios::binary | std::ios::ate);
			if (!f) throw Error(RMD_ERR_INVALID_ARGUMENT, "cannot read " + rays_path);
			const size_t bytes = (size_t)f.tellg();
			if (bytes % (RMD_RAY_DOUBLES * sizeof(double)) != 0)
				throw Error(RMD_ERR_INVALID_ARGUMENT, rays_path + ": " + std::to_string(bytes) + " bytes is no whole number of 48-byte rays");
			if (bytes / (RMD_RAY_DOUBLES * sizeof(double)) > RMD_MAX_RAYS) throw Error(RMD_ERR_INVALID_ARGUMENT, rays_path + ": more than RMD_MAX_RAYS rays");
			std::vector<double> rays(bytes / sizeof(double));
			f.seekg(0);
			if (!rays.empty() && !f.read(reinterpret_cast<char *>(rays.data()), (std::streamsize)bytes)) throw Error(RMD_ERR_INVALID_ARGUMENT, "cannot read " + rays_path);
			const std::vector<rmd_ray_hit> hits = rays.empty() ? std::vector<rmd_ray_hit>() : intersect_rays(scene_of(argv[2]), rays, 0);
			std::ofstream o(out_path, std::ios::binary);
			o.write(reinterpret_cast<const char *>(hits.data()), (std::streamsize)(hits.size() * sizeof(rmd_ray_hit)));
			if (!o) throw Error(RMD_ERR_INVALID_ARGUMENT, "cannot write " + out_path);
			size_t n_hit = 0;
			for (const rmd_ray_hit &h : hits) n_hit += h.object >= 0;
			std::printf("%zu rays, %zu hits\n", hits.size(), n_hit);
			return 0;
		}
		if (argc >= 2 && !std::strcmp(argv[1], "pick")) {
			if (argc < 3 || (argc - 3) % 2 != 0) throw Error(RMD_ERR_INVALID_ARGUMENT, "pick: SCENE --pixel X,Y [--size W,H] [--fov DEGREES] [--position X,Y,Z]");
			Settings st;
			st.camera_settings.backbuffer_width = 1920, st.camera_settings.backbuffer_height = 1080;
			st.camera_settings.fov_vert = 55.0, st.camera_settings.focal_length = 2.5;
			std::vector<uint32_t> pixel;
			for (int i = 3; i + 1 < argc; i += 2) {
				if (!std::strcmp(argv[i], "--pixel")) pixel = parse_u32s("--pixel", argv[i + 1], 2);
				else if (!std::strcmp(argv[i], "--size")) {
					const std::vector<uint32_t> size = parse_u32s("--size", argv[i + 1], 2);
					st.camera_settings.backbuffer_width = size[0], st.camera_settings.backbuffer_height = size[1];
				} else if (!std::strcmp(argv[i], "--fov")) st.camera_settings.fov_vert = parse_doubles("--fov", argv[i + 1], 1)[0];
				else if (!std::strcmp(argv[i], "--position")) {
					const std::vector<double> at = parse_doubles("--position", argv[i + 1], 3);
					st.camera_settings.transform.position = {at[0], at[1], at[2]};
				} else throw Error(RMD_ERR_INVALID_ARGUMENT, std::string("pick: unknown option ") + argv[i]);
			}
			if (pixel.empty()) throw Error(RMD_ERR_INVALID_ARGUMENT, "pick: --pixel X,Y is needed");
			const size_t W = st.camera_settings.backbuffer_width, H = st.camera_settings.backbuffer_height;
			if (W == 0 || H == 0 || W > 65535 || H > 65535) throw Error(RMD_ERR_INVALID_ARGUMENT, "pick: --size must be 1..65535 per axis");
			if (pixel[0] >= W || pixel[1] >= H) throw Error(RMD_ERR_INVALID_ARGUMENT, "pick: pixel outside the frame");
			const rmd_ray_hit h = pick(scene_of(argv[2]), st, pixel[0], pixel[1], 0);
			std::printf("%d %u %.17g %.17g %.17g %.17g\n", h.object, h.triangle, h.t, h.normal[0], h.normal[1], h.normal[2]);
			return 0;
		}
		if (argc >= 5 && !std::strcmp(argv[1], "display-weights")) {
			for (double w : display_weights(std::strtod(argv[2], nullptr), std::strtod(argv[3], nullptr), std::strtod(argv[4], nullptr))) {
				uint64_t bits;
				std::memcpy(&bits, &w, sizeof(bits));
				std::printf("%016llx\n", (unsigned long long)bits);
			}
			return 0;
		}
		if (argc >= 9 && !std::strcmp(argv[1], "tile-weighted-error")) {
			const size_t W = (size_t)std::atoll(argv[4]), H = (size_t)std::atoll(argv[5]);
			std::vector<Vector3> sums(W * H), sums_sq(W * H);
			for (int i = 0; i < 2; i++) {
				std::ifstream f(argv[2 + i], std::ios::binary);
				std::vector<Vector3> &dst = i ? sums_sq : sums;
				if (!f || !f.read(reinterpret_cast<char *>(dst.data()), (std::streamsize)(dst.size() * sizeof(Vector3))))
					throw Error(RMD_ERR_INVALID_ARGUMENT, std::string("cannot read ") + argv[2 + i]);
			}
			std::vector<rmd_tile_rect> rects;
			std::vector<uint32_t> counts;
			std::ifstream rf(argv[6]);
			for (rmd_tile_rect r; rf >> r.left >> r.top >> r.width >> r.height;) {
				uint32_t n = 0;
				rf >> n;
				rects.push_back(r), counts.push_back(n);
			}
			std::vector<double> weights(RMD_LUMA_WEIGHTS);
			if (!std::strcmp(argv[7], "--weights")) {
				std::ifstream f(argv[8], std::ios::binary);
				if (!f || !f.read(reinterpret_cast<char *>(weights.data()), (std::streamsize)(weights.size() * sizeof(double))))
					throw Error(RMD_ERR_INVALID_ARGUMENT, std::string("cannot read ") + argv[8]);
			} else {
				if (argc < 10) throw Error(RMD_ERR_INVALID_ARGUMENT, "tile-weighted-error: EXPOSURE GAMMA FLOOR or --weights FILE");
				weights = display_weights(std::strtod(argv[7], nullptr), std::strtod(argv[8], nullptr), std::strtod(argv[9], nullptr));
			}
			for (const rmd_tile_weighted &t : tile_weighted_error_host(sums, sums_sq, W, H, rects, counts, weights)) {
				uint64_t bits[4];
				const double fields[4] = {t.rms, t.mean_weighted_variance, t.mean_luma, t.mean_variance};
				std::memcpy(bits, fields, sizeof(bits));
				std::printf("%016llx %016llx %016llx %016llx %u %u\n", (unsigned long long)bits[0], (unsigned long long)bits[1], (unsigned long long)bits[2],
				            (unsigned long long)bits[3], t.valid, t.invalid);
			}
			return 0;
		}
		if (argc >= 9 && !std::strcmp(argv[1], "tile-weighted-error-dual")) {
			const size_t W = (size_t)std::atoll(argv[4]), H = (size_t)std::atoll(argv[5]);
			std::vector<Vector3> out(W * H);
			std::vector<double> err(W * H);
			{
				std::ifstream f(argv[2], std::ios::binary), g(argv[3], std::ios::binary);
				if (!f || !f.read(reinterpret_cast<char *>(out.data()), (std::streamsize)(out.size() * sizeof(Vector3)))) throw Error(RMD_ERR_INVALID_ARGUMENT, std::string("cannot read ") + argv[2]);
				if (!g || !g.read(reinterpret_cast<char *>(err.data()), (std::streamsize)(err.size() * sizeof(double)))) throw Error(RMD_ERR_INVALID_ARGUMENT, std::string("cannot read ") + argv[3]);
			}
			std::vector<rmd_tile_rect> rects;
			std::ifstream rf(argv[6]);
			for (rmd_tile_rect r; rf >> r.left >> r.top >> r.width >> r.height;) {
				uint32_t n = 0;
				rf >> n; // (the sibling's count column: read and ignored)
				rects.push_back(r);
			}
			std::vector<double> weights(RMD_LUMA_WEIGHTS);
			if (!std::strcmp(argv[7], "--weights")) {
				std::ifstream f(argv[8], std::ios::binary);
				if (!f || !f.read(reinterpret_cast<char *>(weights.data()), (std::streamsize)(weights.size() * sizeof(double))))
					throw Error(RMD_ERR_INVALID_ARGUMENT, std::string("cannot read ") + argv[8]);
			} else {
				if (argc < 10) throw Error(RMD_ERR_INVALID_ARGUMENT, "tile-weighted-error-dual: EXPOSURE GAMMA FLOOR or --weights FILE");
				weights = display_weights(std::strtod(argv[7], nullptr), std::strtod(argv[8], nullptr), std::strtod(argv[9], nullptr));
			}
			for (const rmd_tile_weighted &t : tile_weighted_error_dual_host(out, err, W, H, rects, weights)) {
				uint64_t bits[4];
				const double fields[4] = {t.rms, t.mean_weighted_variance, t.mean_luma, t.mean_variance};
				std::memcpy(bits, fields, sizeof(bits));
				std::printf("%016llx %016llx %016llx %016llx %u %u\n", (unsigned long long)bits[0], (unsigned long long)bits[1], (unsigned long long)bits[2],
				            (unsigned long long)bits[3], t.valid, t.invalid);
			}
			return 0;
		}
		if (argc >= 6 && !std::strcmp(argv[1], "tiles")) {
			for (const rmd_tile_rect &t : generate_tiles(std::atoi(argv[2]), std::atoi(argv[3]), {std::atoi(argv[4]), std::atoi(argv[5])}))
				std::printf("%u %u %u %u\n", t.left, t.top, t.width, t.height);
			return 0;
		}
		if (argc >= 8 && !std::strcmp(argv[1], "hostapi")) {
			// The measurement bench.py's `host_api` block reports: the scene is built first (as cli_old does, main.rs:45-127), a tiny untimed render
			// initialises the process's HIP runtime, then ONE render_tiled call is timed from the call to the last TileFinished message, the
			// TileProgressed snapshots handed to a callback as they arrive (src/trace.rs:119-134).
			std::string what = argv[2];
			Settings st;
			st.camera_settings.backbuffer_width = std::atoi(argv[3]), st.camera_settings.backbuffer_height = std::atoi(argv[4]);
			st.camera_settings.fov_vert = 55.0, st.camera_settings.focal_length = 2.5;
			st.sample_count = std::atoi(argv[5]), st.bounce_limit = std::atoi(argv[6]), st.samples_per_iteration = std::atoi(argv[7]);
			st.tile_size = {32, 32};
			for (int i = 8; i + 1 < argc; i += 2)
				if (!std::strcmp(argv[i], "--end-black-paths")) st.end_black_paths = std::atoi(argv[i + 1]) != 0;
				else if (!std::strcmp(argv[i], "--preview-every")) st.preview_every = (size_t)std::strtoull(argv[i + 1], nullptr, 10);
				else if (!std::strcmp(argv[i], "--preview-denoise")) st.preview_denoise = std::atoi(argv[i + 1]) != 0;
				else if (!std::strcmp(argv[i], "--progress-tiles")) st.progress_tiles = std::atoi(argv[i + 1]) != 0;
			Scene scene = what == "spheres" ? reflective_spheres() : gold_dragon_standin(what.size() > 7 ? std::atoi(what.c_str() + 7) : 91);
			{
				Settings warm = st;
				warm.camera_settings.backbuffer_width = warm.camera_settings.backbuffer_height = 64, warm.sample_count = 1, warm.samples_per_iteration = 0, warm.preview_every = 0, warm.preview_denoise = false;
				render_tiled(reflective_spheres(), warm).await();
			}
			const int reps = 3;
			double best = 1e30, best_setup = 0.0, best_await = 0.0;
			size_t progressed = 0, finished_tiles = 0, previews = 0;
			double checksum = 0.0;
			for (int rep = 0; rep < reps; rep++) {
				progressed = 0;
				const auto t0 = std::chrono::steady_clock::now();
				TaskHandle handle = render_tiled(scene, st);
				// wall: call -> the last TileFinished message has ARRIVED at the consumer (every message taken through poll() as it comes); then the
				// image is assembled as await() would (:93-99) and the workers' teardown is waited for
				double secs = 0.0;
				std::vector<Vector3> image = consume(handle, st, progressed, &secs, t0, nullptr, nullptr, nullptr, "", &previews);
				const double secs_await = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
				if (secs < best) best = secs, best_setup = handle.setup_seconds(), best_await = secs_await;
				checksum = 0.0;
				for (const Vector3 &v : image)
					for (double c : v)
						if (c == c) checksum += c;
				finished_tiles = generate_tiles(st.camera_settings.backbuffer_width, st.camera_settings.backbuffer_height, st.tile_size).size();
			}
			const double n = (double)st.camera_settings.backbuffer_width * st.camera_settings.backbuffer_height * st.sample_count;
			std::printf("{\"scene\": \"%s\", \"width\": %zu, \"height\": %zu, \"spp\": %zu, \"bounces\": %zu, \"samples_per_iteration\": %zu, \"wall_ms\": %.3f, "
			            "\"setup_ms\": %.3f, \"image_assembled_ms\": %.3f, \"msamples_per_s\": %.2f, \"msamples_per_s_after_setup\": %.2f, \"tile_progressed_messages\": %zu, \"tiles\": %zu, "
			            "\"mean_radiance_sum\": %.17g, \"runs\": %d%s}\n",
			            what.c_str(), st.camera_settings.backbuffer_width, st.camera_settings.backbuffer_height, st.sample_count, st.bounce_limit, st.samples_per_iteration,
			            best * 1e3, best_setup * 1e3, best_await * 1e3, n / best / 1e6, n / (best - best_setup) / 1e6, progressed, finished_tiles, checksum, reps,
			            st.preview_every ? (", \"frame_previews\": " + std::to_string(previews)).c_str() : ""); // (a run without previews prints the line it always printed)
			return 0;
		}
		if (argc >= 8 && !std::strcmp(argv[1], "render")) {
			const auto t0 = std::chrono::steady_clock::now(); // cli_old/src/main.rs:36
			std::string what = argv[2], raw, dump_features, preview_prefix, dump_tiles, dump_ids, dump_matte, matte_objects, dump_ao;
			double ao_distance = 0.0, ao_empty = 1.0;
			bool auto_exposure = false;
			Settings st;
			st.camera_settings.backbuffer_width = std::atoi(argv[3]);
			st.camera_settings.backbuffer_height = std::atoi(argv[4]);
			st.camera_settings.fov_vert = 55.0, st.camera_settings.focal_length = 2.5; // :134-141
			st.sample_count = std::atoi(argv[5]);
			st.bounce_limit = std::atoi(argv[6]);
			st.tile_size = {32, 32}; // :147
			for (int i = 8; i + 1 < argc; i += 2) {
				if (!std::strcmp(argv[i], "--raw")) raw = argv[i + 1];
				else if (!std::strcmp(argv[i], "--gpus")) st.worker_count = std::atoi(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--spi")) st.samples_per_iteration = std::atoi(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--aperture")) st.camera_settings.aperture_radius = std::atof(argv[i + 1]), st.use_dof = true;
				else if (!std::strcmp(argv[i], "--end-black-paths")) st.end_black_paths = std::atoi(argv[i + 1]) != 0; // opt-in on mesh scenes (raymond_hip.h)
				else if (!std::strcmp(argv[i], "--adaptive")) st.adaptive_threshold = std::atof(argv[i + 1]); // (render_tiled refuses it without --spi)
				else if (!std::strcmp(argv[i], "--adaptive-floor")) st.adaptive_floor = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--adaptive-measure")) st.adaptive_measure = argv[i + 1]; // (render_tiled checks it)
				else if (!std::strcmp(argv[i], "--adaptive-display")) st.adaptive_display_threshold = std::atof(argv[i + 1]); // (render_tiled checks them)
				else if (!std::strcmp(argv[i], "--adaptive-display-exposure")) st.adaptive_display_exposure = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--adaptive-display-gamma")) st.adaptive_display_gamma = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--adaptive-display-floor")) st.adaptive_display_floor = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--adaptive-display-auto-exposure")) st.adaptive_display_auto_exposure = std::atoi(argv[i + 1]) != 0;
				else if (!std::strcmp(argv[i], "--dump-tiles")) dump_tiles = argv[i + 1];
				else if (!std::strcmp(argv[i], "--tile-size")) st.tile_size = {(size_t)std::strtoull(argv[i + 1], nullptr, 10), (size_t)std::strtoull(argv[i + 1], nullptr, 10)};
				else if (!std::strcmp(argv[i], "--denoise"))st.denoise = std::atoi(argv[i + 1]) != 0;
				else if (!std::strcmp(argv[i], "--denoise-radius")) st.denoise_radius = (uint32_t)std::strtoul(argv[i + 1], nullptr, 10); // (render_tiled checks them)
				else if (!std::strcmp(argv[i], "--denoise-patch")) st.denoise_patch = (uint32_t)std::strtoul(argv[i + 1], nullptr, 10);
				else if (!std::strcmp(argv[i], "--denoise-k")) st.denoise_k = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--denoise-alpha")) st.denoise_alpha = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--denoise-dual")) st.denoise_dual = std::atoi(argv[i + 1]) != 0;
				else if (!std::strcmp(argv[i], "--denoise-dual-features")) st.denoise_dual_features = std::atoi(argv[i + 1]) != 0;
				else if (!std::strcmp(argv[i], "--denoise-dual-select")) st.denoise_dual_select = std::atoi(argv[i + 1]) != 0;
				else if (!std::strcmp(argv[i], "--denoise-dual-atrous")) st.denoise_dual_atrous = std::atoi(argv[i + 1]) != 0;
				else if (!std::strcmp(argv[i], "--denoise-dual-atrous-region")) st.denoise_dual_atrous_region = std::atoi(argv[i + 1]) != 0;
				else if (!std::strcmp(argv[i], "--adaptive-denoised")) st.adaptive_denoised_threshold = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--adaptive-denoised-display")) st.adaptive_denoised_display_threshold = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--adaptive-min")) st.adaptive_min_samples = (size_t)std::strtoull(argv[i + 1], nullptr, 10);
				else if (!std::strcmp(argv[i], "--denoise-features")) st.denoise_features = std::atoi(argv[i + 1]) != 0;
				else if (!std::strcmp(argv[i], "--denoise-feature-k")) st.denoise_feature_k = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--denoise-feature-tau")) st.denoise_feature_tau = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--denoise-feature-slope")) st.denoise_feature_slope = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--denoise-atrous-slope")) st.denoise_atrous_slope = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--denoise-atrous")) st.denoise_atrous = std::atoi(argv[i + 1]) != 0;
				else if (!std::strcmp(argv[i], "--denoise-atrous-levels")) st.denoise_atrous_levels = (uint32_t)std::strtoul(argv[i + 1], nullptr, 10); // (render_tiled checks them)
				else if (!std::strcmp(argv[i], "--denoise-atrous-k")) st.denoise_atrous_k = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--dump-ids")) dump_ids = argv[i + 1];
				else if (!std::strcmp(argv[i], "--dump-matte")) dump_matte = argv[i + 1];
				else if (!std::strcmp(argv[i], "--matte-objects")) matte_objects = argv[i + 1];
				else if (!std::strcmp(argv[i], "--dump-ao")) dump_ao = argv[i + 1];
				else if (!std::strcmp(argv[i], "--ao-distance")) ao_distance = std::strtod(argv[i + 1], nullptr); // (inf: any hit)
				else if (!std::strcmp(argv[i], "--ao-empty")) ao_empty = std::strtod(argv[i + 1], nullptr);
				else if (!std::strcmp(argv[i], "--dump-features")) dump_features = argv[i + 1];
				else if (!std::strcmp(argv[i], "--preview-every")) st.preview_every = (size_t)std::strtoull(argv[i + 1], nullptr, 10); // (render_tiled refuses it without --spi)
				else if (!std::strcmp(argv[i], "--preview-prefix")) preview_prefix = argv[i + 1];
				else if (!std::strcmp(argv[i], "--preview-denoise")) st.preview_denoise = std::atoi(argv[i + 1]) != 0;
				else if (!std::strcmp(argv[i], "--preview-exposure")) st.preview_exposure = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--preview-gamma")) st.preview_gamma = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--progress-tiles")) st.progress_tiles = std::atoi(argv[i + 1]) != 0;
				else if (!std::strcmp(argv[i], "--auto-exposure")) auto_exposure = std::atoi(argv[i + 1]) != 0;
				else if (!std::strcmp(argv[i], "--auto-exposure-percentile")) st.auto_exposure_percentile = std::atof(argv[i + 1]); // (render_tiled checks them)
				else if (!std::strcmp(argv[i], "--auto-exposure-target")) st.auto_exposure_target = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--despike")) st.despike = std::atoi(argv[i + 1]) != 0;
				else if (!std::strcmp(argv[i], "--despike-dual")) st.despike_dual = std::atoi(argv[i + 1]) != 0;
				else if (!std::strcmp(argv[i], "--despike-radius")) st.despike_radius = (uint32_t)std::atoi(argv[i + 1]); // (render_tiled checks them)
				else if (!std::strcmp(argv[i], "--despike-rank")) st.despike_rank = (uint32_t)std::atoi(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--despike-k")) st.despike_k = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--despike-ratio")) st.despike_ratio = std::atof(argv[i + 1]);
				else if (!std::strcmp(argv[i], "--despike-floor")) st.despike_floor = std::atof(argv[i + 1]);
			}
			const bool want_ao = !dump_ao.empty(); // (--dump-ao: the finished tiles' rects and counts, as for --dump-ids)
			if (want_ao && !(ao_distance > 0.0)) throw Error(RMD_ERR_INVALID_ARGUMENT, "--dump-ao needs --ao-distance D with D > 0"); // (before anything is rendered)
			st.preview_auto_exposure = auto_exposure && st.preview_every > 0; // (a render without previews: the final frame alone)
			Scene scene;
			if (what == "spheres") scene = reflective_spheres();
			else if (what.rfind("dragon", 0) == 0) scene = gold_dragon_standin(what.size() > 7 ? std::atoi(what.c_str() + 7) : 91);
			else if (what.rfind("project:", 0) == 0) scene = Project::load(what.substr(8)).build_scene(); // core/src/project.rs
			else throw Error(RMD_ERR_INVALID_ARGUMENT, "unknown scene " + what);
			TaskHandle handle = render_tiled(scene, st); // :152
			size_t progressed = 0;
			// progressive mode: every message is taken as it arrives (consume); else await() (:153)
			// (--dump-features: every message is taken by consume, which keeps the finished tiles' rects and counts)
			std::vector<double> feature_means;
			std::vector<Tile> finished;
			const bool want_ids = !dump_ids.empty() || !dump_matte.empty(); // (--dump-ids / --dump-matte: the finished tiles' rects and counts likewise)
			const std::vector<uint32_t> matte_set = parse_objects(matte_objects);
			const bool by_consume = st.samples_per_iteration != 0 || !dump_features.empty() || !dump_tiles.empty() || want_ids || want_ao;
			std::vector<Vector3> image = by_consume ? consume(handle, st, progressed, nullptr, t0, &scene, dump_features.empty() ? nullptr : &feature_means, &finished, preview_prefix)
			                                        : handle.await();
			const size_t W = st.camera_settings.backbuffer_width, H = st.camera_settings.backbuffer_height;
			if (!dump_features.empty()) {
				if (feature_means.empty()) { // not a guided render: a feature pass of its own over the finished tiles, each at its count
					std::vector<rmd_tile_rect> rects;
					std::vector<uint32_t> counts;
					for (const Tile &t : finished) {
						rects.push_back(rect_of(t));
						counts.push_back((uint32_t)t.sample_count);
					}
					feature_means = render_features(scene, st, rects, counts, 0);
					divide_by_counts(feature_means, W, H, RMD_FEATURE_CHANNELS, rects, counts);
				}
				std::ofstream f(dump_features, std::ios::binary);
				f.write(reinterpret_cast<const char *>(feature_means.data()), (std::streamsize)(feature_means.size() * 8));
			}
			if (want_ids) { // an ID pass of its own over the finished tiles, each at its count
				std::vector<rmd_tile_rect> rects;
				std::vector<uint32_t> counts;
				for (const Tile &t : finished) {
					rects.push_back(rect_of(t));
					counts.push_back((uint32_t)t.sample_count);
				}
				const std::vector<uint32_t> words = render_ids(scene, st, rects, counts, 0);
				if (!dump_ids.empty()) {
					std::ofstream f(dump_ids, std::ios::binary);
					f.write(reinterpret_cast<const char *>(words.data()), (std::streamsize)(words.size() * sizeof(uint32_t)));
				}
				if (!dump_matte.empty()) {
					uint64_t other = 0;
					const std::vector<double> matte = ids_matte(words, W, H, matte_set, 0, &other);
					std::ofstream f(dump_matte, std::ios::binary);
					f.write(reinterpret_cast<const char *>(matte.data()), (std::streamsize)(matte.size() * 8));
					std::printf("matte: %llu pixels with other != 0\n", (unsigned long long)other);
				}
			}
			if (want_ao) { // an AO pass of its own over the finished tiles, each at its count
				std::vector<rmd_tile_rect> rects;
				std::vector<uint32_t> counts;
				for (const Tile &t : finished) {
					rects.push_back(rect_of(t));
					counts.push_back((uint32_t)t.sample_count);
				}
				uint64_t empty = 0;
				const std::vector<double> out = ao_resolve(render_ao(scene, st, rects, counts, ao_distance, 0), W, H, ao_empty, 0, &empty);
				std::ofstream f(dump_ao, std::ios::binary);
				f.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)(out.size() * 8));
				std::printf("ao: %llu pixels without a first hit\n", (unsigned long long)empty);
			}
			if (!dump_tiles.empty()) { // the finished tiles in the order they arrived: which tile stopped at which count, and by what error
				std::ofstream f(dump_tiles);
				char line[128];
				for (const Tile &t : finished) {
					std::snprintf(line, sizeof(line), "%zu %zu %zu %zu %zu %.17g\n", t.left, t.top, t.width, t.height, t.sample_count, t.error);
					f << line;
				}
			}
			double exposure = 1.0; // :165
			if (auto_exposure) { // the final frame is on the host already: its histogram is made here, with the lines the device's kernel is built from
				const rmd_luma_histogram hist = luminance_histogram(image);
				if (rmd_exposure_from_histogram(&hist, st.auto_exposure_percentile, st.auto_exposure_target, &exposure) != RMD_OK)
					throw Error(RMD_ERR_INVALID_ARGUMENT, rmd_last_error(nullptr));
				std::printf("auto exposure: %.17g\n", exposure);
			}
			write_ppm(argv[7], tone_map(image, exposure), W, H); // :161-197
			if (!raw.empty()) {
				std::ofstream f(raw, std::ios::binary);
				f.write(reinterpret_cast<const char *>(image.data()), (std::streamsize)(image.size() * 24));
			}
			const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
			std::printf("Finished render.\nTotal render time: %.3fs\n%zu x %zu, %zu spp, %zu bounces: %.1f Msamples/s end to end\n", secs, W, H, st.sample_count,
			            st.bounce_limit, (double)W * H * st.sample_count / secs / 1e6);
			return 0;
		}
		std::fprintf(stderr, "usage: see the header of raymond_amd/host/cli.cpp\n");
		return 2;
	} catch (const std::exception &e) {
		std::fprintf(stderr, "raymond_cli: %s\n", e.what());
		return 1;
	}
}
