// Implementation of raymond.hpp (host side above the C-ABI).  Host code only: every pixel is produced by
// rmd_render_tiles; nothing here evaluates a ray.
#include "raymond.hpp"

#include "../csrc/ao_rule.hpp"
#include "../csrc/despike_dual_rule.hpp"
#include "../csrc/despike_rule.hpp"
#include "../csrc/ids_rule.hpp"
#include "../csrc/luma_bins.hpp"
#include "../csrc/tile_luma_rule.hpp"
#include "../csrc/tile_weighted_dual_rule.hpp"
#include "../csrc/tile_weighted_rule.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <tuple>
#include <utility>

namespace raymond {

namespace {
void check(rmd_status s, rmd_context *ctx, const char *what) {
	if (s != RMD_OK) {
		const char *text = rmd_last_error(ctx);
		throw Error(s, std::string(what) + ": " + (text ? text : ""));
	}
}
} // namespace

// ---------------------------------------------------------------- Mesh (core/src/geometry/mesh.rs)
Mesh Mesh::load_ply(const std::string &path) {
	std::ifstream in(path);
	if (!in) throw Error(RMD_ERR_INVALID_ARGUMENT, "load_ply: cannot open " + path); // reference: unwrap() panic
	std::string line;
	size_t n_vertices = 0;
	// header (:66-77): only `element vertex N` matters
	while (std::getline(in, line)) {
		std::istringstream tok(line);
		std::string a, b;
		if (!(tok >> a)) throw Error(RMD_ERR_INVALID_ARGUMENT, "load_ply: empty header line"); // tokens.next().unwrap()
		if (a == "element") {
			tok >> b;
			if (b == "vertex") tok >> n_vertices;
		} else if (a == "end_header") {
			break;
		}
	}
	struct V {
		double p[3], n[3];
	};
	std::vector<V> verts;
	verts.reserve(n_vertices);
	for (size_t i = 0; i < n_vertices; i++) { // :80-90
		if (!std::getline(in, line)) throw Error(RMD_ERR_INVALID_ARGUMENT, "load_ply: vertex list truncated");
		std::istringstream tok(line);
		std::vector<double> v;
		double x;
		while (tok >> x) v.push_back(x);
		if (v.size() < 6) throw Error(RMD_ERR_INVALID_ARGUMENT, "load_ply: vertex line with fewer than 6 values");
		verts.push_back(V{{v[0], v[1], v[2]}, {v[3], v[4], v[5]}}); // uv (:87) and tangent (:88,:101-108) are not on the hot path
	}
	Mesh m;
	while (std::getline(in, line)) { // :93-118
		std::istringstream tok(line);
		std::vector<unsigned long> v;
		unsigned long x;
		while (tok >> x) v.push_back(x);
		if (v.empty()) throw Error(RMD_ERR_INVALID_ARGUMENT, "load_ply: empty face line"); // values[0] panics
		if (v[0] != 3) continue;                                                            // non-triangles are dropped (:116)
		if (v.size() < 4) throw Error(RMD_ERR_INVALID_ARGUMENT, "load_ply: triangle with fewer than 3 indices");
		for (int k = 1; k <= 3; k++) {
			if (v[k] >= verts.size()) throw Error(RMD_ERR_INVALID_ARGUMENT, "load_ply: vertex index out of range");
			for (int a = 0; a < 3; a++) m.tri_pos.push_back(verts[v[k]].p[a]);
		}
		for (int k = 1; k <= 3; k++)
			for (int a = 0; a < 3; a++) m.tri_nrm.push_back(verts[v[k]].n[a]);
	}
	return m;
}

void Mesh::bake_transform(Vector3 t) {
	for (size_t i = 0; i < tri_pos.size(); i++) tri_pos[i] += t[i % 3];
}

// ---------------------------------------------------------------- AccGrid
std::shared_ptr<AccGrid> AccGrid::build_from_mesh(const Mesh &mesh) {
	std::shared_ptr<AccGrid> g(new AccGrid());
	check(rmd_grid_build_from_mesh(mesh.tri_pos.data(), mesh.tri_nrm.data(), mesh.triangle_count(), &g->build_), nullptr, "AccGrid::build_from_mesh");
	check(rmd_grid_build_describe(g->build_, &g->desc_), nullptr, "AccGrid::build_from_mesh");
	return g;
}
AccGrid::~AccGrid() { rmd_grid_build_destroy(build_); }

// ---------------------------------------------------------------- render_tiled
std::vector<rmd_tile_rect> generate_tiles(size_t width, size_t height, std::pair<size_t, size_t> ts) {
	std::vector<rmd_tile_rect> tiles;
	size_t x = 0, y = 0;
	for (;;) {
		size_t x1 = std::min(x + ts.first, width), y1 = std::min(y + ts.second, height);
		tiles.push_back(rmd_tile_rect{(uint32_t)x, (uint32_t)y, (uint32_t)(x1 - x), (uint32_t)(y1 - y)});
		y += ts.second;
		if (y >= height) {
			y = 0;
			x += ts.first;
		}
		if (x >= width) break;
	}
	return tiles;
}

rmd_tile_rect rect_of(const Tile &t) { return rmd_tile_rect{(uint32_t)t.left, (uint32_t)t.top, (uint32_t)t.width, (uint32_t)t.height}; }

void place_tile(const Tile &t, const TileData &data, size_t width, std::vector<Vector3> &frame, double divisor) {
	for (size_t y = 0; y < t.height; y++)
		for (size_t x = 0; x < t.width; x++) {
			Vector3 s = data[x + y * t.width];
			for (double &c : s) c /= divisor; // :95 (x / 1.0 is x: without a divisor the sums arrive as they are)
			frame[x + t.left + (y + t.top) * width] = s;
		}
}

void divide_by_counts(std::vector<double> &sums, size_t width, size_t height, size_t channels, const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts) {
	std::vector<double> n_img(width * height, 0.0);
	for (size_t i = 0; i < rects.size(); i++)
		for (size_t y = rects[i].top; y < (size_t)rects[i].top + rects[i].height; y++)
			for (size_t x = rects[i].left; x < (size_t)rects[i].left + rects[i].width; x++) n_img[x + y * width] = (double)counts[i];
	for (size_t p = 0; p < width * height; p++)
		for (size_t j = 0; j < channels; j++) sums[p * channels + j] /= n_img[p];
}

struct TaskHandle::Shared {
	std::mutex m;
	std::condition_variable cv;
	std::deque<Tile> queue;      // MsQueue<Tile> (:138)
	std::deque<Message> channel; // mpsc::channel (:139)
	size_t alive = 0;            // alive_thread_count (:175)
	size_t in_flight = 0;        // tiles popped by a worker and not yet finished or re-queued
	std::string error;
	double setup_s = 0.0;        // measurement: the longest a worker took to get ready (context, scene upload, framebuffer)
};

namespace {

void flatten(const Scene &scene, std::vector<rmd_object> &objs, std::vector<rmd_grid_desc> &grids) {
	std::vector<const AccGrid *> seen;
	for (const Object &o : scene.objects) {
		rmd_object r;
		std::memset(&r, 0, sizeof(r));
		r.geometry_kind = o.geometry.kind;
		if (o.geometry.kind == RMD_GEOM_PLANE) {
			for (int a = 0; a < 3; a++) r.origin[a] = o.geometry.plane.origin[a], r.normal[a] = o.geometry.plane.normal[a];
		} else if (o.geometry.kind == RMD_GEOM_SPHERE) {
			for (int a = 0; a < 3; a++) r.origin[a] = o.geometry.sphere.origin[a];
			r.radius = o.geometry.sphere.radius;
		} else {
			const AccGrid *g = o.geometry.grid.get();
			size_t gi = std::find(seen.begin(), seen.end(), g) - seen.begin();
			if (gi == seen.size()) {
				seen.push_back(g);
				grids.push_back(g->desc());
			}
			r.grid_index = (uint32_t)gi;
		}
		r.material.kind = o.material.kind;
		for (int a = 0; a < 3; a++) r.material.color[a] = o.material.color[a];
		r.material.roughness = o.material.roughness;
		for (int a = 0; a < 5; a++) r.material.emission_aux[a] = o.material.aux[a];
		objs.push_back(r);
	}
}

// ---------------------------------------------------------------- owners of what the C-ABI hands out
// Move-only, freed by their destructors.  Whoever holds several declares them context, scene, frames: they then go frames first, the context last.
class Context {
  public:
	explicit Context(int device) { check(rmd_context_create(device, &p_), nullptr, "rmd_context_create"); }
	~Context() { rmd_context_destroy(p_); }
	Context(Context &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
	Context &operator=(Context &&) = delete;
	operator rmd_context *() const { return p_; }

  private:
	rmd_context *p_ = nullptr;
};

class DeviceScene { // a Scene flattened and uploaded to a context's GPU
  public:
	DeviceScene(rmd_context *ctx, const Scene &scene) {
		std::vector<rmd_object> objs;
		std::vector<rmd_grid_desc> grids;
		flatten(scene, objs, grids);
		check(rmd_scene_create(ctx, objs.data(), (uint32_t)objs.size(), grids.data(), (uint32_t)grids.size(), &p_), ctx, "rmd_scene_create");
	}
	~DeviceScene() { rmd_scene_destroy(p_); }
	DeviceScene(DeviceScene &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
	DeviceScene &operator=(DeviceScene &&) = delete;
	operator rmd_scene *() const { return p_; }

  private:
	rmd_scene *p_ = nullptr;
};

class Frame { // a zeroed W x H device buffer of sums: 3 doubles a pixel, the features' RMD_FEATURE_CHANNELS, an ID buffer's 5 (RMD_ID_WORDS words), or an AO buffer's 2 (RMD_AO_WORDS words) — or W * H rays (6 doubles each) or hit records (5); empty (a null pointer) until one is moved in
  public:
	enum Kind { Colour, Features, Ids, Ao, Rays, Hits };
	Frame() = default;
	Frame(rmd_context *ctx, size_t W, size_t H, Kind kind = Colour) : ctx_(ctx) {
		if (kind == Features) check(rmd_feature_buffer_alloc(ctx, (uint32_t)W, (uint32_t)H, &p_), ctx, "rmd_feature_buffer_alloc");
		else if (kind == Ids) check(rmd_id_buffer_alloc(ctx, (uint32_t)W, (uint32_t)H, reinterpret_cast<uint32_t **>(&p_)), ctx, "rmd_id_buffer_alloc");
		else if (kind == Ao) check(rmd_ao_buffer_alloc(ctx, (uint32_t)W, (uint32_t)H, reinterpret_cast<uint32_t **>(&p_)), ctx, "rmd_ao_buffer_alloc");
		else if (kind == Rays) check(rmd_ray_buffer_alloc(ctx, (uint64_t)W * H, &p_), ctx, "rmd_ray_buffer_alloc");
		else if (kind == Hits) check(rmd_hit_buffer_alloc(ctx, (uint64_t)W * H, reinterpret_cast<rmd_ray_hit **>(&p_)), ctx, "rmd_hit_buffer_alloc");
		else check(rmd_framebuffer_alloc(ctx, (uint32_t)W, (uint32_t)H, &p_), ctx, "rmd_framebuffer_alloc");
	}
	~Frame() {
		if (p_) rmd_framebuffer_free(ctx_, p_);
	}
	Frame(Frame &&o) noexcept : ctx_(o.ctx_), p_(std::exchange(o.p_, nullptr)) {}
	Frame &operator=(Frame &&o) noexcept {
		std::swap(ctx_, o.ctx_), std::swap(p_, o.p_);
		return *this;
	}
	operator double *() const { return p_; }

  private:
	rmd_context *ctx_ = nullptr;
	double *p_ = nullptr;
};

// ---------------------------------------------------------------- the C-ABI's PODs from a Settings, and the small sums
rmd_camera camera_pod(const Settings &st) {
	rmd_camera cam;
	std::memset(&cam, 0, sizeof(cam));
	cam.backbuffer_width = (uint32_t)st.camera_settings.backbuffer_width, cam.backbuffer_height = (uint32_t)st.camera_settings.backbuffer_height;
	cam.fov_vert = st.camera_settings.fov_vert;
	for (int a = 0; a < 3; a++) cam.position[a] = st.camera_settings.transform.position[a];
	cam.focal_length = st.camera_settings.focal_length, cam.aperture_radius = st.camera_settings.aperture_radius;
	return cam;
}
uint32_t feature_flags(const Settings &st) { return st.use_dof ? RMD_RENDER_DOF : 0u; } // what rmd_render_features takes: the DOF flag alone
uint32_t render_flags(const Settings &st) { // 0 = the reference's loop: pinhole (:199), every sample identical
	return feature_flags(st) | (st.end_black_paths ? RMD_RENDER_END_BLACK_PATHS : 0u);
}
rmd_settings settings_pod(const Settings &st, size_t begin, size_t n, uint32_t flags) { // samples [begin, begin + n)
	rmd_settings rs;
	std::memset(&rs, 0, sizeof(rs));
	rs.bounce_limit = (uint32_t)st.bounce_limit, rs.sample_begin = (uint32_t)begin, rs.sample_count = (uint32_t)n, rs.seed = st.seed, rs.flags = flags;
	return rs;
}
size_t pixels_of(const std::vector<rmd_tile_rect> &rects) {
	size_t pixels = 0;
	for (const rmd_tile_rect &r : rects) pixels += (size_t)r.width * r.height;
	return pixels;
}
std::vector<uint32_t> sum_counts(const std::vector<uint32_t> &a, const std::vector<uint32_t> &b) {
	std::vector<uint32_t> both(a);
	for (size_t i = 0; i < both.size(); i++) both[i] += b[i];
	return both;
}
std::vector<rmd_tile_rect> rects_of(const std::vector<Tile> &tiles, const std::vector<size_t> &which) {
	std::vector<rmd_tile_rect> rects;
	for (size_t i : which) rects.push_back(rect_of(tiles[i]));
	return rects;
}

// Page-locked blocks for the downloads, recycled: a block goes back to the pool when the last tile (message) that views it is dropped.
struct BlockPool : std::enable_shared_from_this<BlockPool> {
	static std::shared_ptr<BlockPool> shared() {
		static std::shared_ptr<BlockPool> pool = std::make_shared<BlockPool>();
		return pool;
	}
	std::mutex m;
	std::vector<std::pair<void *, size_t>> free_blocks;
	// (the blocks of the process-wide pool are left to the operating system at exit: the HIP runtime may be gone by then)
	std::shared_ptr<void> get(rmd_context *ctx, size_t bytes) {
		void *p = nullptr;
		size_t have = 0;
		{
			std::lock_guard<std::mutex> lock(m);
			for (size_t i = 0; i < free_blocks.size(); i++)
				if (free_blocks[i].second >= bytes) {
					p = free_blocks[i].first, have = free_blocks[i].second;
					free_blocks.erase(free_blocks.begin() + (long)i);
					break;
				}
		}
		if (!p) {
			check(rmd_host_alloc(ctx, bytes, &p), ctx, "rmd_host_alloc");
			have = bytes;
		}
		std::shared_ptr<BlockPool> self = shared_from_this();
		return std::shared_ptr<void>(p, [self, have](void *q) {
			std::lock_guard<std::mutex> lock(self->m);
			if (self->free_blocks.size() < 4) self->free_blocks.emplace_back(q, have);
			else rmd_host_free(nullptr, q);
		});
	}
};

void scatter_packed(const std::vector<rmd_tile_rect> &rects, const uint8_t *packed, size_t packed_bytes, size_t width, size_t height, std::vector<uint8_t> &frame) {
	frame.resize(width * height * 3, 0);
	size_t at = 0;
	for (const rmd_tile_rect &r : rects) {
		const size_t row = (size_t)r.width * 3;
		if ((size_t)r.left + r.width > width || (size_t)r.top + r.height > height || at + row * r.height > packed_bytes)
			throw Error(RMD_ERR_INVALID_ARGUMENT, "scatter_tiles: a rect outside the frame, or fewer packed bytes than the rects hold");
		for (size_t y = 0; y < r.height; y++, at += row) std::memcpy(frame.data() + ((size_t)r.left + ((size_t)r.top + y) * width) * 3, packed + at, row);
	}
}

// One FramePreview message: the rects of `fb` (plus `fb2`'s sums when it is not null), each at its count, resolved and tone-mapped on the GPU and scattered
// into a frame
Message preview_message(rmd_context *ctx, const double *fb, const double *fb2, size_t W, size_t H, const std::vector<rmd_tile_rect> &rects,
                        const std::vector<uint32_t> &counts, const Settings &st, size_t pass_index, size_t sample_count) {
	auto pv = std::make_shared<Preview>();
	pv->width = W, pv->height = H, pv->pass_index = pass_index, pv->sample_count = sample_count;
	// the packed bytes arrive in a page-locked block of the pool the tile downloads use, as those do
	const size_t pixels = pixels_of(rects);
	std::shared_ptr<void> block = BlockPool::shared()->get(ctx, std::max<size_t>(pixels * 3, 1));
	double exposure = st.preview_exposure;
	if (st.preview_auto_exposure) { // the histogram of exactly what the resolve call below takes
		rmd_luma_histogram hist;
		check(rmd_luminance_histogram_tiles(ctx, fb, fb2, (uint32_t)W, (uint32_t)H, rects.data(), counts.data(), (uint32_t)rects.size(), &hist), ctx,
		      "rmd_luminance_histogram_tiles");
		check(rmd_exposure_from_histogram(&hist, st.auto_exposure_percentile, st.auto_exposure_target, &exposure), nullptr, "rmd_exposure_from_histogram");
		pv->exposure = exposure;
	}
	check(rmd_resolve_tonemap_tiles(ctx, fb, fb2, (uint32_t)W, (uint32_t)H, rects.data(), counts.data(), (uint32_t)rects.size(), exposure, st.preview_gamma,
	                                static_cast<uint8_t *>(block.get())),
	      ctx, "rmd_resolve_tonemap_tiles");
	scatter_packed(rects, static_cast<const uint8_t *>(block.get()), pixels * 3, W, H, pv->rgb8);
	Message m;
	m.kind = Message::FramePreview, m.preview = std::move(pv);
	return m;
}

// The dual-buffer filter that `st` selects, as its one C-ABI call: over the two halves half[0..3] = S_A, Q_A, S_B, Q_B of a W x H frame whose rect i holds
// counts_a[i] + counts_b[i] samples, into `out` and — where it is not null — the error image `err`.  feat / feat_sq: the feature sums and sums of squares
// at those counts added, or nulls.  region (n_region rects), or null: the caller reads only those pixels of `out` and `err` — the adaptive check of the
// dual loop, whose region is its live tiles; the forms that have a region form then write those pixels alone, with the whole-frame call's bytes.
//   denoise_dual_atrous:   rmd_denoise_atrous_dual, guided where the features are given; its region form only with denoise_dual_atrous_region
//   denoise_dual_select:   rmd_denoise_dual_select at the setting's two candidates (it needs the features)
//   the features given:    rmd_denoise_dual_guided[_region]
//   otherwise:             rmd_denoise_dual[_region]
// With denoise_feature_slope > 0 the second and the third are their _slope calls (the guided candidate's slope; the setting excludes the first).
// With denoise_atrous_slope > 0 and the features given the first is rmd_denoise_atrous_dual_slope[_region].
// Two things that a reader may take for oversights and that every caller's bytes depend on: a call with a region never selects — rmd_denoise_dual_select
// has no region form, and a select render's adaptive check is the plain or the guided region form —; and the unguided call with a region is
// rmd_denoise_dual_region where the one without is rmd_denoise_dual.
void denoise_dual_frame(rmd_context *ctx, const Settings &st, size_t W, size_t H, const Frame *half, const double *feat, const double *feat_sq,
                        const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts_a, const std::vector<uint32_t> &counts_b, const rmd_tile_rect *region,
                        size_t n_region, double *out, double *err) {
	const uint32_t w = (uint32_t)W, h = (uint32_t)H, n = (uint32_t)rects.size(), nr = (uint32_t)n_region;
	const std::vector<uint32_t> counts_f = sum_counts(counts_a, counts_b); // (not read without the features)
	const uint32_t *ca = counts_a.data(), *cb = counts_b.data(), *cf = counts_f.data();
	if (st.denoise_dual_atrous && feat && st.denoise_atrous_slope > 0.0 && region && st.denoise_dual_atrous_region) {
		check(rmd_denoise_atrous_dual_slope_region(ctx, half[0], half[1], half[2], half[3], feat, feat_sq, w, h, rects.data(), ca, cb, cf, n, region, nr, st.denoise_atrous_levels,
		                                           st.denoise_atrous_k, st.denoise_alpha, st.denoise_feature_k, st.denoise_feature_tau, st.denoise_atrous_slope, out, err),
		      ctx, "rmd_denoise_atrous_dual_slope_region");
	} else if (st.denoise_dual_atrous && feat && st.denoise_atrous_slope > 0.0) {
		check(rmd_denoise_atrous_dual_slope(ctx, half[0], half[1], half[2], half[3], feat, feat_sq, w, h, rects.data(), ca, cb, cf, n, st.denoise_atrous_levels, st.denoise_atrous_k,
		                                    st.denoise_alpha, st.denoise_feature_k, st.denoise_feature_tau, st.denoise_atrous_slope, out, err),
		      ctx, "rmd_denoise_atrous_dual_slope");
	} else if (st.denoise_dual_atrous && region && st.denoise_dual_atrous_region) {
		check(rmd_denoise_atrous_dual_region(ctx, half[0], half[1], half[2], half[3], feat, feat_sq, w, h, rects.data(), ca, cb, cf, n, region, nr, st.denoise_atrous_levels,
		                                     st.denoise_atrous_k, st.denoise_alpha, st.denoise_feature_k, st.denoise_feature_tau, out, err),
		      ctx, "rmd_denoise_atrous_dual_region");
	} else if (st.denoise_dual_atrous) {
		check(rmd_denoise_atrous_dual(ctx, half[0], half[1], half[2], half[3], feat, feat_sq, w, h, rects.data(), ca, cb, cf, n, st.denoise_atrous_levels, st.denoise_atrous_k,
		                              st.denoise_alpha, st.denoise_feature_k, st.denoise_feature_tau, out, err),
		      ctx, "rmd_denoise_atrous_dual");
	} else if (st.denoise_dual_select && !region && st.denoise_feature_slope > 0.0) {
		const rmd_denoise_candidate cands[2] = {{st.denoise_k, st.denoise_alpha, 0.0, 0.0, 0u, 0u}, {1.0, st.denoise_alpha, st.denoise_feature_k, st.denoise_feature_tau, 1u, 0u}};
		const double slopes[2] = {0.0, st.denoise_feature_slope}; // (the guided candidate's)
		check(rmd_denoise_dual_select_slope(ctx, half[0], half[1], half[2], half[3], feat, feat_sq, w, h, rects.data(), ca, cb, cf, n, st.denoise_radius, st.denoise_patch, cands,
		                                    slopes, 2u, 2u, 2u, out, err, nullptr, nullptr),
		      ctx, "rmd_denoise_dual_select_slope");
	} else if (st.denoise_dual_select && !region) {
		const rmd_denoise_candidate cands[2] = {{st.denoise_k, st.denoise_alpha, 0.0, 0.0, 0u, 0u}, {1.0, st.denoise_alpha, st.denoise_feature_k, st.denoise_feature_tau, 1u, 0u}};
		check(rmd_denoise_dual_select(ctx, half[0], half[1], half[2], half[3], feat, feat_sq, w, h, rects.data(), ca, cb, cf, n, st.denoise_radius, st.denoise_patch, cands, 2u,
		                              2u, 2u, out, err, nullptr, nullptr),
		      ctx, "rmd_denoise_dual_select");
	} else if (feat && region && st.denoise_feature_slope > 0.0) {
		check(rmd_denoise_dual_guided_slope_region(ctx, half[0], half[1], half[2], half[3], feat, feat_sq, w, h, rects.data(), ca, cb, cf, n, region, nr, st.denoise_radius,
		                                           st.denoise_patch, st.denoise_k, st.denoise_alpha, st.denoise_feature_k, st.denoise_feature_tau, st.denoise_feature_slope, out,
		                                           err),
		      ctx, "rmd_denoise_dual_guided_slope_region");
	} else if (feat && st.denoise_feature_slope > 0.0) {
		check(rmd_denoise_dual_guided_slope(ctx, half[0], half[1], half[2], half[3], feat, feat_sq, w, h, rects.data(), ca, cb, cf, n, st.denoise_radius, st.denoise_patch,
		                                    st.denoise_k, st.denoise_alpha, st.denoise_feature_k, st.denoise_feature_tau, st.denoise_feature_slope, out, err),
		      ctx, "rmd_denoise_dual_guided_slope");
	} else if (feat && region) {
		check(rmd_denoise_dual_guided_region(ctx, half[0], half[1], half[2], half[3], feat, feat_sq, w, h, rects.data(), ca, cb, cf, n, region, nr, st.denoise_radius,
		                                     st.denoise_patch, st.denoise_k, st.denoise_alpha, st.denoise_feature_k, st.denoise_feature_tau, out, err),
		      ctx, "rmd_denoise_dual_guided_region");
	} else if (feat) {
		check(rmd_denoise_dual_guided(ctx, half[0], half[1], half[2], half[3], feat, feat_sq, w, h, rects.data(), ca, cb, cf, n, st.denoise_radius, st.denoise_patch, st.denoise_k,
		                              st.denoise_alpha, st.denoise_feature_k, st.denoise_feature_tau, out, err),
		      ctx, "rmd_denoise_dual_guided");
	} else if (region) {
		check(rmd_denoise_dual_region(ctx, half[0], half[1], half[2], half[3], w, h, rects.data(), ca, cb, n, region, nr, st.denoise_radius, st.denoise_patch, st.denoise_k,
		                              st.denoise_alpha, out, err),
		      ctx, "rmd_denoise_dual_region");
	} else {
		check(rmd_denoise_dual(ctx, half[0], half[1], half[2], half[3], w, h, rects.data(), ca, cb, n, st.denoise_radius, st.denoise_patch, st.denoise_k, st.denoise_alpha, out,
		                       err),
		      ctx, "rmd_denoise_dual");
	}
}

// What both kinds of worker hold while they run: their GPU's context, the scene on it, and what every launch takes.  The frames are the derived
// structs' members, so they are freed first, then the scene, then the context.
struct Worker {
	TaskHandle::Shared &sh;
	const Settings st;
	const size_t W, H;
	Context ctx;
	DeviceScene dscene;
	const rmd_camera cam;
	const uint32_t flags;
	Worker(TaskHandle::Shared &sh, int device, const Scene &scene, const Settings &st)
	    : sh(sh), st(st), W(st.camera_settings.backbuffer_width), H(st.camera_settings.backbuffer_height), ctx(device), dscene(ctx, scene), cam(camera_pod(st)),
	      flags(render_flags(st)) {}
	Frame frame(bool wanted = true, Frame::Kind kind = Frame::Colour) { return wanted ? Frame(ctx, W, H, kind) : Frame(); } // zeroed: a fresh tile's sums
};

// One worker = one GPU.  Pops a batch of tiles, adds `step` samples to each with ONE rmd_render_tiles call per sample count, then reports them
// finished or re-queues them (src/trace.rs:188-221).  The tiles' sums stay in this GPU's framebuffer; only what a message carries is downloaded,
// on the copy stream, while the next batch renders (the messages of batch k are sent while batch k + 1 runs).
struct TileWorker : Worker {
	const int me;
	const size_t workers, batch;
	// previews (one worker: render_tiled): every batch is then one pass over all live tiles, which all hold the same count
	const bool preview, preview_filtered, adaptive, moments;
	const bool luma_measure;  // settings.adaptive_measure is "luma_tile" or "luma_pixel": the check is rmd_tile_luma_error
	const bool display_measure; // settings.adaptive_display_threshold > 0: the check is rmd_tile_weighted_error under the tone curve's weights
	const double threshold;     // what a tile's measure has to meet: adaptive_display_threshold with the display measure, else adaptive_threshold
	std::vector<double> weights; // display_measure: rmd_display_weights' table — made once, or with adaptive_display_auto_exposure by every check
	const bool despike_check; // settings.despike in an adaptive render (one worker: check_settings): the check reads despiked copies of the sums
	const size_t step;
	Frame fb, fb_sq;    // fb_sq: the sums of squares of an adaptive, denoised or despiked render
	Frame fb_preview;   // settings.preview_denoise: the filtered means of a preview
	Frame fb_spare, fb_spare_sq; // despike_check: rmd_despike's outputs, which rmd_tile_error reads; fb and fb_sq stay raw
	std::vector<rmd_tile_rect> converged_rects; // despike_check, adaptive_display_auto_exposure: the tiles that finished early and the counts they finished with
	std::vector<uint32_t> converged_counts;
	std::shared_ptr<BlockPool> pool = BlockPool::shared(); // process-wide: page-locking 50 MB costs about as much as moving them
	std::vector<rmd_tile_rect> early_rects; // previews: the tiles that finished early and the counts they finished with
	std::vector<uint32_t> early_counts;
	size_t passes = 0;
	// a batch whose download is on its way: the tiles that become messages, in message order
	struct Pending {
		std::vector<Message> messages;
		std::vector<Tile> requeue; // (several workers: tiles that go back to the queue with their sums in RAM)
		size_t taken = 0;          // tiles of the batch that were neither finished nor re-queued at once (they leave `in_flight` now)
	};
	std::optional<Pending> pending;
	struct Fate {
		bool finished, progressed; // the tile is done (:211-212); it goes on and this pass sends a snapshot of it (:217-219)
	};

	TileWorker(TaskHandle::Shared &sh, int device, int me, size_t workers, const Scene &scene, const Settings &st, size_t batch)
	    : Worker(sh, device, scene, st), me(me), workers(workers), batch(batch), preview(st.preview_every > 0), preview_filtered(preview && st.preview_denoise),
	      adaptive(st.adaptive_threshold > 0.0 || st.adaptive_display_threshold > 0.0), moments(adaptive || st.denoise || preview_filtered || st.despike),
	      luma_measure(st.adaptive_measure != "channel_max"), display_measure(st.adaptive_display_threshold > 0.0),
	      threshold(display_measure ? st.adaptive_display_threshold : st.adaptive_threshold),
	      weights(display_measure ? display_weights(st.adaptive_display_exposure, st.adaptive_display_gamma, st.adaptive_display_floor) : std::vector<double>()),
	      despike_check(st.despike && adaptive),
	      step(st.samples_per_iteration ? st.samples_per_iteration : st.sample_count), fb(frame()), fb_sq(frame(moments)), fb_preview(frame(preview_filtered)),
	      fb_spare(frame(despike_check)), fb_spare_sq(frame(despike_check)) {}

	void run() {
		for (;;) {
			std::vector<Tile> mine = take_batch();
			if (mine.empty()) break;
			passes++;
			upload_arrivals(mine);
			launch(mine);
			flush(); // the previous batch's messages go out while this batch renders
			const std::vector<Fate> fate = decide(mine);
			start_downloads(mine, fate);
			Pending next;
			std::vector<Tile> resident_requeue;
			sort_batch(mine, fate, next, resident_requeue);
			if (preview) add_preview(next, resident_requeue);
			publish(resident_requeue, std::move(next));
		}
		flush();
		check(rmd_context_synchronize(ctx), ctx, "rmd_context_synchronize"); // a device fault of the last launch surfaces here at the latest
	}

	void flush() { // the previous batch's download has to arrive before its messages can be sent
		if (!pending) return;
		check(rmd_context_wait_transfers(ctx), ctx, "rmd_context_wait_transfers");
		std::lock_guard<std::mutex> lock(sh.m);
		for (Message &m : pending->messages) sh.channel.push_back(std::move(m));
		for (Tile &t : pending->requeue) sh.queue.push_back(std::move(t));
		sh.in_flight -= pending->taken;
		pending.reset();
		sh.cv.notify_all();
	}

	std::vector<Tile> take_batch() {
		// try_pop (:189).  The reference's worker leaves as soon as the queue is empty (:191-194); with one GPU call
		// per batch a queue that is only momentarily empty — the other workers hold every tile and will re-queue them
		// for the next progressive pass — would collapse the pool to one GPU, so a worker leaves only when no tile is
		// queued AND none is in flight.
		std::vector<Tile> mine;
		std::unique_lock<std::mutex> lock(sh.m);
		if (sh.queue.empty() && pending) { // nothing to start: send what is pending (it may re-queue tiles or end the render)
			lock.unlock();
			flush();
			lock.lock();
		}
		sh.cv.wait(lock, [&] { return !sh.queue.empty() || sh.in_flight == 0 || !sh.error.empty(); });
		while (sh.error.empty() && !sh.queue.empty() && mine.size() < batch) {
			mine.push_back(std::move(sh.queue.front()));
			sh.queue.pop_front();
		}
		sh.in_flight += mine.size();
		return mine;
	}

	// tiles that arrive with their sums in RAM (another GPU rendered their earlier passes): into this GPU's framebuffer
	void upload_arrivals(const std::vector<Tile> &mine) {
		std::vector<rmd_tile_rect> rects;
		std::vector<double> packed, packed_sq;
		for (const Tile &t : mine)
			if (t.resident != me && t.sample_count != 0) {
				rects.push_back(rect_of(t));
				const double *src = reinterpret_cast<const double *>(t.data.data());
				packed.insert(packed.end(), src, src + t.data.size() * 3);
				if (moments) {
					const double *sq = reinterpret_cast<const double *>(t.data_sq.data());
					packed_sq.insert(packed_sq.end(), sq, sq + t.data_sq.size() * 3);
				}
			}
		if (!rects.empty()) check(rmd_framebuffer_upload_tiles(ctx, packed.data(), fb, (uint32_t)W, (uint32_t)H, rects.data(), (uint32_t)rects.size()), ctx, "rmd_framebuffer_upload_tiles");
		if (!rects.empty() && moments)
			check(rmd_framebuffer_upload_tiles(ctx, packed_sq.data(), fb_sq, (uint32_t)W, (uint32_t)H, rects.data(), (uint32_t)rects.size()), ctx, "rmd_framebuffer_upload_tiles");
	}

	// tiles of one batch may be at different sample counts: one launch per count (enqueued, not waited for)
	void launch(std::vector<Tile> &mine) {
		std::map<size_t, std::vector<size_t>> by_count;
		for (size_t i = 0; i < mine.size(); i++) by_count[mine[i].sample_count].push_back(i);
		for (auto &grp : by_count) {
			const size_t begin = grp.first, n = std::min(step, st.sample_count - begin);
			const std::vector<rmd_tile_rect> rects = rects_of(mine, grp.second);
			const rmd_settings rs = settings_pod(st, begin, n, flags);
			if (moments) check(rmd_render_tiles_moments_async(ctx, dscene, &cam, &rs, rects.data(), (uint32_t)rects.size(), fb, fb_sq), ctx, "rmd_render_tiles_moments");
			else check(rmd_render_tiles_async(ctx, dscene, &cam, &rs, rects.data(), (uint32_t)rects.size(), fb), ctx, "rmd_render_tiles");
			for (size_t i : grp.second) mine[i].sample_count += n, mine[i].resident = me, mine[i].data = TileData(), mine[i].data_sq = TileData(); // :207 — the sums are on this GPU now
		}
	}

	// adaptive: the error of every tile this pass has left below sample_count, one rmd_tile_error per sample count (it waits for the pass); a
	// tile at or below the threshold is finished at the samples it has
	// With a luma measure (settings.adaptive_measure): ONE rmd_tile_luma_error over all of them, each rect at its own count; its tile_rms or pixel_rms
	// decides and stays with the tile as `error`
	// With the display measure (settings.adaptive_display_threshold): ONE rmd_tile_weighted_error over all of them, each rect at its own count, under
	// rmd_display_weights' table; with adaptive_display_auto_exposure the table is first made anew from the histogram of the whole frame — the tiles that
	// finished early at their counts and the batch, which with one worker is every other tile — on the sums the check reads
	// What converged_tiles hands to the library: rects (or the indices in `mine` of the tiles they are cut from) and each one's count
	struct Counted {
		std::vector<size_t> which;
		std::vector<rmd_tile_rect> rects;
		std::vector<uint32_t> counts;
	};
	// the tiles below sample_count at their counts, which the luma and the display measure take in one call
	Counted below_sample_count(const std::vector<Tile> &mine) const {
		Counted c;
		for (size_t i = 0; i < mine.size(); i++)
			if (mine[i].sample_count < st.sample_count) c.which.push_back(i), c.counts.push_back((uint32_t)mine[i].sample_count);
		c.rects = rects_of(mine, c.which);
		return c;
	}
	// every tile at its current count, which rmd_despike and the histogram take: the tiles that finished early, then `mine`
	Counted finished_and_current(const std::vector<Tile> &mine) const {
		Counted c;
		c.rects = converged_rects, c.counts = converged_counts;
		for (const Tile &t : mine) c.rects.push_back(rect_of(t)), c.counts.push_back((uint32_t)t.sample_count);
		return c;
	}
	std::vector<bool> converged_tiles(std::vector<Tile> &mine) {
		std::vector<bool> converged(mine.size(), false);
		if (!adaptive) return converged;
		std::map<size_t, std::vector<size_t>> live;
		for (size_t i = 0; i < mine.size(); i++)
			if (mine[i].sample_count < st.sample_count) live[mine[i].sample_count].push_back(i);
		const double *s = fb, *s_sq = fb_sq;
		if (despike_check && !live.empty()) {
			// one worker: the batch is every tile that has not finished.  All tiles at their current counts go through rmd_despike into the spare buffers
			const Counted all = finished_and_current(mine);
			check(rmd_despike(ctx, fb, fb_sq, (uint32_t)W, (uint32_t)H, all.rects.data(), all.counts.data(), (uint32_t)all.rects.size(), st.despike_radius, st.despike_rank, st.despike_k,
			                  st.despike_ratio, st.despike_floor, fb_spare, fb_spare_sq, nullptr),
			      ctx, "rmd_despike");
			s = fb_spare, s_sq = fb_spare_sq;
		}
		if (display_measure && !live.empty()) {
			if (st.adaptive_display_auto_exposure) {
				const Counted all = finished_and_current(mine);
				rmd_luma_histogram hist;
				check(rmd_luminance_histogram_tiles(ctx, s, nullptr, (uint32_t)W, (uint32_t)H, all.rects.data(), all.counts.data(), (uint32_t)all.rects.size(), &hist), ctx,
				      "rmd_luminance_histogram_tiles");
				double exposure = 1.0;
				check(rmd_exposure_from_histogram(&hist, st.auto_exposure_percentile, st.auto_exposure_target, &exposure), nullptr, "rmd_exposure_from_histogram");
				weights = display_weights(exposure, st.adaptive_display_gamma, st.adaptive_display_floor);
			}
			const Counted b = below_sample_count(mine);
			std::vector<rmd_tile_weighted> weighted(b.rects.size());
			check(rmd_tile_weighted_error(ctx, s, s_sq, (uint32_t)W, (uint32_t)H, b.rects.data(), b.counts.data(), (uint32_t)b.rects.size(), weights.data(), weighted.data()), ctx,
			      "rmd_tile_weighted_error");
			for (size_t k = 0; k < weighted.size(); k++) mine[b.which[k]].error = weighted[k].rms, converged[b.which[k]] = weighted[k].rms <= threshold;
			live.clear(); // (no rmd_tile_error call below)
		}
		if (luma_measure) {
			const Counted b = below_sample_count(mine);
			std::vector<rmd_tile_luma> luma(b.rects.size());
			if (!b.rects.empty())
				check(rmd_tile_luma_error(ctx, s, s_sq, (uint32_t)W, (uint32_t)H, b.rects.data(), b.counts.data(), (uint32_t)b.rects.size(), st.adaptive_floor, luma.data()), ctx,
				      "rmd_tile_luma_error");
			for (size_t k = 0; k < luma.size(); k++) {
				const double e = st.adaptive_measure == "luma_tile" ? luma[k].tile_rms : luma[k].pixel_rms;
				mine[b.which[k]].error = e, converged[b.which[k]] = e <= threshold;
			}
			live.clear(); // (no rmd_tile_error call below)
		}
		for (auto &grp : live) {
			const std::vector<rmd_tile_rect> rects = rects_of(mine, grp.second);
			std::vector<double> err(rects.size());
			check(rmd_tile_error(ctx, s, s_sq, (uint32_t)W, (uint32_t)H, (uint32_t)grp.first, st.adaptive_floor, rects.data(), (uint32_t)rects.size(), err.data()), ctx,
			      "rmd_tile_error");
			for (size_t k = 0; k < err.size(); k++) converged[grp.second[k]] = err[k] <= threshold;
		}
		if (despike_check || (display_measure && st.adaptive_display_auto_exposure))
			for (size_t i = 0; i < mine.size(); i++)
				if (converged[i]) converged_rects.push_back(rect_of(mine[i])), converged_counts.push_back((uint32_t)mine[i].sample_count);
		return converged;
	}

	std::vector<Fate> decide(std::vector<Tile> &mine) {
		const std::vector<bool> converged = converged_tiles(mine);
		std::vector<Fate> fate(mine.size());
		for (size_t i = 0; i < mine.size(); i++) {
			const bool finished = mine[i].sample_count == st.sample_count || converged[i];
			fate[i] = Fate{finished, !finished && st.progress_tiles && st.samples_per_iteration != 0 && mine[i].sample_count % st.samples_per_iteration == 0};
		}
		return fate;
	}

	// the tiles `want` of `from`, enqueued on the copy stream into one block of the pool; `field` of each of them becomes its view of that block
	void download(const Frame &from, std::vector<Tile> &mine, const std::vector<size_t> &want, TileData Tile::*field) {
		if (want.empty()) return;
		const std::vector<rmd_tile_rect> rects = rects_of(mine, want);
		std::shared_ptr<void> block = pool->get(ctx, pixels_of(rects) * 24);
		check(rmd_framebuffer_download_tiles_async(ctx, from, (uint32_t)W, (uint32_t)H, rects.data(), (uint32_t)rects.size(), static_cast<double *>(block.get())), ctx,
		      "rmd_framebuffer_download_tiles");
		Vector3 *p = static_cast<Vector3 *>(block.get());
		for (size_t i : want) {
			mine[i].*field = TileData(block, p, mine[i].width * mine[i].height);
			p += mine[i].width * mine[i].height;
		}
	}

	// what of this batch has to come to the host: finished tiles (:211-212), progress snapshots (:217-219), and — with several GPUs — every
	// tile that goes back to the shared queue (another GPU may take it next)
	void start_downloads(std::vector<Tile> &mine, const std::vector<Fate> &fate) {
		std::vector<size_t> want;
		// the sums of squares: of the tiles that go back to the shared queue (adaptive or denoised, several GPUs) and of the finished tiles (denoised)
		std::vector<size_t> want_sq;
		for (size_t i = 0; i < mine.size(); i++) {
			if (fate[i].finished || fate[i].progressed || workers > 1) want.push_back(i);
			if ((moments && !fate[i].finished && workers > 1) || ((st.denoise || st.despike) && fate[i].finished)) want_sq.push_back(i);
		}
		download(fb, mine, want, &Tile::data);
		download(fb_sq, mine, want_sq, &Tile::data_sq);
	}

	void sort_batch(std::vector<Tile> &mine, const std::vector<Fate> &fate, Pending &next, std::vector<Tile> &resident_requeue) {
		for (size_t i = 0; i < mine.size(); i++) {
			Tile &t = mine[i];
			if (fate[i].finished) {
				t.resident = -1;
				next.messages.push_back(Message{Message::TileFinished, std::move(t)});
				next.taken++;
			} else if (workers > 1) { // back to the shared queue with its sums in RAM, once they have arrived
				t.resident = -1;
				if (fate[i].progressed) {
					Tile snapshot = t;
					snapshot.data_sq = TileData(); // (the sums of squares stay with the scheduler)
					next.messages.push_back(Message{Message::TileProgressed, std::move(snapshot)});
				}
				next.requeue.push_back(std::move(t));
				next.taken++;
			} else { // one GPU: the tile goes back to the queue at once, sums resident; its snapshot follows when it has arrived
				if (fate[i].progressed) {
					Tile snapshot = t;
					snapshot.resident = -1;
					next.messages.push_back(Message{Message::TileProgressed, std::move(snapshot)});
				}
				t.data = TileData();
				resident_requeue.push_back(std::move(t));
			}
		}
	}

	// behind this pass's messages: the whole frame, the tiles that go on at this pass's count, those that finished early at their own
	void add_preview(Pending &next, const std::vector<Tile> &resident_requeue) {
		const size_t done = resident_requeue.empty() ? st.sample_count : resident_requeue.front().sample_count;
		for (const Message &m : next.messages)
			if (m.kind == Message::TileFinished && m.tile.sample_count < st.sample_count) {
				early_rects.push_back(rect_of(m.tile));
				early_counts.push_back((uint32_t)m.tile.sample_count);
			}
		if (resident_requeue.empty() || passes % st.preview_every != 0) return;
		std::vector<rmd_tile_rect> rects(early_rects);
		std::vector<uint32_t> counts(early_counts);
		for (const Tile &t : resident_requeue) rects.push_back(rect_of(t));
		counts.insert(counts.end(), resident_requeue.size(), (uint32_t)done);
		const double *src = fb;
		if (preview_filtered) {
			check(rmd_denoise_atrous(ctx, fb, fb_sq, nullptr, nullptr, (uint32_t)W, (uint32_t)H, rects.data(), counts.data(), (uint32_t)rects.size(), st.denoise_atrous_levels,
			                         st.denoise_atrous_k, st.denoise_alpha, st.denoise_feature_k, st.denoise_feature_tau, fb_preview),
			      ctx, "rmd_denoise_atrous");
			src = fb_preview, counts.assign(rects.size(), 1u); // (means)
		}
		next.messages.push_back(preview_message(ctx, src, nullptr, W, H, rects, counts, st, passes, done));
	}

	void publish(std::vector<Tile> &resident_requeue, Pending &&next) {
		{
			std::lock_guard<std::mutex> lock(sh.m);
			sh.in_flight -= resident_requeue.size();
			for (Tile &t : resident_requeue) sh.queue.push_back(std::move(t));
			sh.cv.notify_all();
		}
		pending = std::move(next);
	}
};

// settings.denoise_dual: the one worker of a dual-buffer render, a plain loop over passes (every live tile takes every pass).  Four framebuffers:
// pass j, counted from 0, adds its samples to half A (fbs 0, 1) when j is even and to half B (fbs 2, 3) when j is odd.  With
// adaptive_denoised_threshold > 0, after every even number of passes that leaves the live tiles below sample_count with at least
// adaptive_min_samples: rmd_denoise_dual_region over the live tiles' pixels of the whole frame (finished tiles at the counts they finished with),
// rmd_tile_error_dual over the live tiles, and the tiles at or below the threshold are finished.  Progress snapshots go out as they are made, the finished tiles at the end.
// With denoise_dual_features the adaptive check needs the features: two feature buffers, into which every pass also adds the live tiles' first-hit
// features of its samples [done, done + n) — a tile's features then hold count_a + count_b samples —, and the check is rmd_denoise_dual_guided_region.
// With denoise_dual_atrous the check is rmd_denoise_atrous_dual on the whole frame, at the same rects, counts and feature buffers; with
// denoise_dual_atrous_region it is rmd_denoise_atrous_dual_region over the live tiles, which gives the pixels read here the same bytes.
struct DualWorker : Worker {
	const bool display; // adaptive_denoised_display_threshold: the check is rmd_tile_weighted_error_dual under the tone curve's weights
	const bool adaptive;
	const double threshold; // what a tile's measure has to meet
	std::vector<double> weights; // display: rmd_display_weights' table — made once, or with adaptive_display_auto_exposure by every check
	const bool guided; // (without the adaptive check nothing here would read the features: await() renders its own)
	Frame fbs[6];      // S_A, Q_A, S_B, Q_B; adaptive: the filtered frame and the error image
	Frame feat[2];     // guided: the feature sums and sums of squares
	Frame fb_preview;  // settings.preview_denoise: the filtered means of a preview
	Frame spare[4];    // settings.despike_dual, when this loop filters (the check, the filtered preview): rmd_despike_dual's outputs, which every dual filter call here reads; fbs stay raw
	size_t despiked_at = ~(size_t)0; // the pass whose despiked halves `spare` holds
	Settings preview_st; // ... which are always the fast filter's, whichever filter the settings select for the frame: `st` with denoise_dual_atrous on
	std::vector<rmd_tile_rect> live, done_rects;
	std::vector<uint32_t> done_a, done_b;
	std::vector<Message> finished;
	size_t n_half[2] = {0, 0}, done = 0, j = 0;

	DualWorker(TaskHandle::Shared &sh, int device, const Scene &scene, const Settings &st)
	    : Worker(sh, device, scene, st), display(st.adaptive_denoised_display_threshold > 0.0), adaptive(st.adaptive_denoised_threshold > 0.0 || display),
	      threshold(display ? st.adaptive_denoised_display_threshold : st.adaptive_denoised_threshold),
	      weights(display ? display_weights(st.adaptive_display_exposure, st.adaptive_display_gamma, st.adaptive_display_floor) : std::vector<double>()),
	      guided(adaptive && st.denoise_dual_features), preview_st(st),
	      live(generate_tiles(W, H, st.tile_size)) {
		for (int i = 0; i < (adaptive ? 6 : 4); i++) fbs[i] = frame();
		for (Frame &f : feat) f = frame(guided, Frame::Features);
		fb_preview = frame(st.preview_every > 0 && st.preview_denoise);
		for (Frame &f : spare) f = frame(st.despike_dual && (adaptive || fb_preview));
		preview_st.denoise_dual_atrous = true;
	}

	void run() {
		while (done < st.sample_count && !live.empty()) {
			render_pass();
			if (done >= st.sample_count) break;
			const std::vector<double> errors = adaptive_check(); // (empty: this pass is not followed by a check)
			std::vector<rmd_tile_rect> converged, still;
			std::vector<double> converged_err, still_err;
			for (size_t k = 0; k < live.size(); k++) {
				const bool conv = !errors.empty() && errors[k] <= threshold;
				(conv ? converged : still).push_back(live[k]);
				if (!errors.empty()) (conv ? converged_err : still_err).push_back(errors[k]);
			}
			finish(converged, converged_err);
			std::vector<Message> out = snapshots(still, still_err);
			if (!still.empty() && st.preview_every > 0 && j % st.preview_every == 0) out.push_back(preview(still));
			send(out);
			live = std::move(still);
		}
		finish(live, {});
		send(finished);
	}

	void send(std::vector<Message> &messages) {
		std::lock_guard<std::mutex> lock(sh.m);
		for (Message &m : messages) sh.channel.push_back(std::move(m));
		sh.cv.notify_all();
	}

	void render_pass() {
		const size_t n = std::min(st.samples_per_iteration, st.sample_count - done), half = j & 1;
		const rmd_settings rs = settings_pod(st, done, n, flags);
		check(rmd_render_tiles_moments(ctx, dscene, &cam, &rs, live.data(), (uint32_t)live.size(), fbs[2 * half], fbs[2 * half + 1]), ctx, "rmd_render_tiles_moments");
		if (guided) {
			const rmd_settings fs = settings_pod(st, done, n, feature_flags(st));
			check(rmd_render_features(ctx, dscene, &cam, &fs, live.data(), (uint32_t)live.size(), feat[0], feat[1]), ctx, "rmd_render_features");
		}
		done += n, j++, n_half[half] += n;
	}

	// the whole frame: finished tiles at the counts they finished with, `tiles` — the live ones — at n_A and n_B
	struct FrameCounts {
		std::vector<rmd_tile_rect> rects;
		std::vector<uint32_t> a, b;
	};
	FrameCounts whole_frame(const std::vector<rmd_tile_rect> &tiles) const {
		FrameCounts f{done_rects, done_a, done_b};
		f.rects.insert(f.rects.end(), tiles.begin(), tiles.end());
		f.a.insert(f.a.end(), tiles.size(), (uint32_t)n_half[0]), f.b.insert(f.b.end(), tiles.size(), (uint32_t)n_half[1]);
		return f;
	}

	// the halves a dual filter call of this pass reads: the loop's own, or with despike_dual the despiked halves of the whole frame `f`, made once a pass by one
	// rmd_despike_dual call (a later call of the same pass has the same tiles at the same counts)
	const Frame *filter_halves(const FrameCounts &f) {
		if (!spare[0]) return fbs;
		if (despiked_at != j) {
			check(rmd_despike_dual(ctx, fbs[0], fbs[1], fbs[2], fbs[3], (uint32_t)W, (uint32_t)H, f.rects.data(), f.a.data(), f.b.data(), (uint32_t)f.rects.size(), st.despike_radius,
			                       st.despike_rank, st.despike_k, st.despike_ratio, st.despike_floor, spare[0], spare[1], spare[2], spare[3], nullptr),
			      ctx, "rmd_despike_dual");
			despiked_at = j;
		}
		return spare;
	}

	// the live tiles' rmd_tile_error_dual after the filter the settings select; only the live tiles' filtered pixels are read, so they are the filter's region.
	// With adaptive_denoised_display_threshold: one rmd_tile_weighted_error_dual call's rms on the filtered frame and the error image instead; with
	// adaptive_display_auto_exposure the table is first made anew from one histogram of the whole frame's RAW sums — S_A with S_B as the second buffer, at the
	// counts a raw preview of this moment resolves (the region forms leave the filtered frame's finished tiles unwritten)
	std::vector<double> adaptive_check() {
		std::vector<double> errors;
		if (!(adaptive && j % 2 == 0 && done >= st.adaptive_min_samples)) return errors;
		const FrameCounts f = whole_frame(live);
		denoise_dual_frame(ctx, st, W, H, filter_halves(f), feat[0], feat[1], f.rects, f.a, f.b, live.data(), live.size(), fbs[4], fbs[5]);
		errors.resize(live.size());
		if (display) {
			if (st.adaptive_display_auto_exposure) {
				rmd_luma_histogram hist;
				const std::vector<uint32_t> counts = sum_counts(f.a, f.b);
				check(rmd_luminance_histogram_tiles(ctx, fbs[0], fbs[2], (uint32_t)W, (uint32_t)H, f.rects.data(), counts.data(), (uint32_t)f.rects.size(), &hist), ctx,
				      "rmd_luminance_histogram_tiles");
				double exposure = 1.0;
				check(rmd_exposure_from_histogram(&hist, st.auto_exposure_percentile, st.auto_exposure_target, &exposure), nullptr, "rmd_exposure_from_histogram");
				weights = display_weights(exposure, st.adaptive_display_gamma, st.adaptive_display_floor);
			}
			std::vector<rmd_tile_weighted> weighted(live.size());
			check(rmd_tile_weighted_error_dual(ctx, fbs[4], fbs[5], (uint32_t)W, (uint32_t)H, live.data(), (uint32_t)live.size(), weights.data(), weighted.data()), ctx,
			      "rmd_tile_weighted_error_dual");
			for (size_t k = 0; k < weighted.size(); k++) errors[k] = weighted[k].rms;
			return errors;
		}
		check(rmd_tile_error_dual(ctx, fbs[5], (uint32_t)W, (uint32_t)H, live.data(), (uint32_t)live.size(), errors.data()), ctx, "rmd_tile_error_dual");
		return errors;
	}

	// the rects' pixels of one framebuffer, tile after tile in Tile.data layout
	std::vector<Vector3> download(const Frame &fb, const std::vector<rmd_tile_rect> &rects) {
		const size_t pixels = pixels_of(rects);
		std::vector<Vector3> packed(pixels);
		if (pixels)
			check(rmd_framebuffer_download_tiles(ctx, fb, (uint32_t)W, (uint32_t)H, rects.data(), (uint32_t)rects.size(), reinterpret_cast<double *>(packed.data())), ctx,
			      "rmd_framebuffer_download_tiles");
		return packed;
	}

	// the TileFinished messages of `rects` (kept for the end) with both halves; they are in every later check and preview at these counts
	void finish(const std::vector<rmd_tile_rect> &rects, const std::vector<double> &errors) {
		if (rects.empty()) return;
		std::vector<Vector3> packed[4];
		for (int i = 0; i < 4; i++) packed[i] = download(fbs[i], rects);
		size_t at = 0;
		for (size_t k = 0; k < rects.size(); k++) {
			const rmd_tile_rect &r = rects[k];
			const size_t n = (size_t)r.width * r.height;
			Tile t;
			t.left = r.left, t.top = r.top, t.width = r.width, t.height = r.height;
			t.count_a = n_half[0], t.count_b = n_half[1], t.sample_count = n_half[0] + n_half[1];
			if (!errors.empty()) t.error = errors[k];
			TileData *half[4] = {&t.data_a, &t.data_sq_a, &t.data_b, &t.data_sq_b};
			for (int i = 0; i < 4; i++) {
				*half[i] = TileData(n);
				std::copy(packed[i].begin() + (long)at, packed[i].begin() + (long)(at + n), half[i]->data());
			}
			t.data = TileData(n), t.data_sq = TileData(n);
			for (size_t p = 0; p < n; p++)
				for (int c = 0; c < 3; c++) t.data[p][c] = t.data_a[p][c] + t.data_b[p][c], t.data_sq[p][c] = t.data_sq_a[p][c] + t.data_sq_b[p][c];
			at += n;
			finished.push_back(Message{Message::TileFinished, std::move(t)});
			done_rects.push_back(r), done_a.push_back((uint32_t)n_half[0]), done_b.push_back((uint32_t)n_half[1]);
		}
	}

	// progress snapshots of the tiles that go on: the two halves' sums added
	std::vector<Message> snapshots(const std::vector<rmd_tile_rect> &still, const std::vector<double> &still_err) {
		std::vector<Message> out;
		if (!st.progress_tiles) return out;
		const std::vector<Vector3> pa = download(fbs[0], still), pb = download(fbs[2], still);
		size_t at = 0;
		for (size_t k = 0; k < still.size(); k++) {
			const rmd_tile_rect &r = still[k];
			const size_t px = (size_t)r.width * r.height;
			Tile t;
			t.left = r.left, t.top = r.top, t.width = r.width, t.height = r.height, t.sample_count = done;
			if (!still_err.empty()) t.error = still_err[k];
			t.data = TileData(px);
			for (size_t p = 0; p < px; p++)
				for (int c = 0; c < 3; c++) t.data[p][c] = pa[at + p][c] + pb[at + p][c];
			at += px;
			out.push_back(Message{Message::TileProgressed, std::move(t)});
		}
		return out;
	}

	// the whole frame, the two halves' sums added on the device — or, with preview_denoise, the fast filter's means of them, guided when the loop keeps the features
	Message preview(const std::vector<rmd_tile_rect> &still) {
		const FrameCounts f = whole_frame(still);
		if (!fb_preview) return preview_message(ctx, fbs[0], fbs[2], W, H, f.rects, sum_counts(f.a, f.b), st, j, done);
		denoise_dual_frame(ctx, preview_st, W, H, filter_halves(f), feat[0], feat[1], f.rects, f.a, f.b, nullptr, 0, fb_preview, nullptr);
		return preview_message(ctx, fb_preview, nullptr, W, H, f.rects, std::vector<uint32_t>(f.rects.size(), 1u), st, j, done); // (means)
	}
};

// What the two kinds of worker share: make the worker — context, scene, frames — and record how long that took, run it, and whatever happened
// publish the error and leave.  The worker, and with it its device memory, is gone BEFORE alive-- is published: await() takes alive == 0 for
// "torn down", and a consumer of the channel for "the workers free their device memory after their last message".
template <class W, class... Args> void worker_main(std::shared_ptr<TaskHandle::Shared> sh, const Args &...args) {
	try {
		const auto t_setup = std::chrono::steady_clock::now();
		W worker(*sh, args...);
		{
			std::lock_guard<std::mutex> lock(sh->m);
			sh->setup_s = std::max(sh->setup_s, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_setup).count());
		}
		worker.run();
	} catch (const std::exception &e) {
		std::lock_guard<std::mutex> lock(sh->m);
		if (sh->error.empty()) sh->error = e.what(); // the waiting workers see it and leave
		sh->cv.notify_all();
	}
	std::lock_guard<std::mutex> lock(sh->m);
	sh->alive--; // :192
	sh->cv.notify_all();
}

} // namespace

std::string check_preview(const Settings &st) {
	if (st.preview_every > 0 && st.samples_per_iteration == 0) return "preview_every > 0 needs samples_per_iteration > 0 (a preview is made between passes)";
	if (!(st.preview_exposure > 0.0) || !std::isfinite(st.preview_exposure)) return "preview_exposure must be finite and > 0";
	if (!(st.preview_gamma > 0.0) || !std::isfinite(st.preview_gamma)) return "preview_gamma must be finite and > 0";
	if (st.preview_denoise && st.preview_every == 0) return "preview_denoise needs preview_every > 0 (it selects the filter of the previews)";
	if (st.preview_denoise && st.worker_count > 1)
		return "preview_denoise renders on one device: the filter's window crosses the tiles that several devices would own";
	if (st.preview_every > 0 && st.worker_count > 1)
		return "preview_every > 0 needs worker_count == 1 here: a tile moves from GPU to GPU between passes, so no GPU holds a frame's share";
	if (st.preview_auto_exposure && st.preview_every == 0) return "preview_auto_exposure needs preview_every > 0 (it sets the exposure of the previews)";
	if (!(st.auto_exposure_percentile > 0.0 && st.auto_exposure_percentile <= 1.0)) return "auto_exposure_percentile must be finite and in (0, 1]";
	if (!(st.auto_exposure_target > 0.0 && st.auto_exposure_target < 1.0)) return "auto_exposure_target must be finite and in (0, 1)";
	return "";
}

namespace {
// What render_tiled refuses in a Settings: the first failing check's text, or nothing.  The order is part of what a caller sees.
std::string check_settings(const Settings &st) {
	auto positive = [](double v) { return v > 0.0 && std::isfinite(v); };
	if (const std::string why = check_preview(st); !why.empty()) return why;
	if (st.denoise_radius > 12 || st.denoise_patch > 4) return "denoise_radius must be <= 12, denoise_patch <= 4";
	if (!positive(st.denoise_k)) return "denoise_k must be finite and > 0";
	if (!(st.denoise_alpha >= 0.0) || !std::isfinite(st.denoise_alpha)) return "denoise_alpha must be finite and >= 0";
	if (!positive(st.denoise_feature_k)) return "denoise_feature_k must be finite and > 0";
	if (!positive(st.denoise_feature_tau)) return "denoise_feature_tau must be finite and > 0";
	if (st.denoise_features && !st.denoise) return "denoise_features needs denoise";
	if (st.denoise_atrous_levels > RMD_ATROUS_MAX_LEVELS) return "denoise_atrous_levels must be <= 8";
	if (!positive(st.denoise_atrous_k)) return "denoise_atrous_k must be finite and > 0";
	if (st.denoise_atrous && !st.denoise) return "denoise_atrous needs denoise";
	if (st.denoise_atrous && st.denoise_dual) return "denoise_atrous cannot be combined with denoise_dual: rmd_denoise_atrous has no dual form";
	if (!(st.adaptive_threshold >= 0.0)) return "adaptive_threshold must be >= 0 (0 = off)";
	if (st.adaptive_threshold > 0.0 && st.samples_per_iteration == 0) return "adaptive_threshold > 0 needs samples_per_iteration > 0 (the error is checked between passes)";
	if (!positive(st.adaptive_floor)) return "adaptive_floor must be finite and > 0";
	if (st.adaptive_measure != "channel_max" && st.adaptive_measure != "luma_tile" && st.adaptive_measure != "luma_pixel")
		return "adaptive_measure must be \"channel_max\", \"luma_tile\" or \"luma_pixel\"";
	if (!(st.adaptive_display_threshold >= 0.0) || !std::isfinite(st.adaptive_display_threshold)) return "adaptive_display_threshold must be finite and >= 0 (0 = off)";
	if (st.adaptive_display_threshold > 0.0 && st.samples_per_iteration == 0)
		return "adaptive_display_threshold > 0 needs samples_per_iteration > 0 (the error is checked between passes)";
	if (st.adaptive_display_threshold > 0.0 && st.adaptive_threshold > 0.0) return "adaptive_display_threshold and adaptive_threshold are mutually exclusive";
	if (st.adaptive_display_threshold > 0.0 && st.adaptive_measure != "channel_max")
		return "adaptive_display_threshold cannot be combined with adaptive_measure: the display rule is a measure of its own";
	if (!positive(st.adaptive_display_exposure)) return "adaptive_display_exposure must be finite and > 0";
	if (!positive(st.adaptive_display_gamma)) return "adaptive_display_gamma must be finite and > 0";
	if (!(st.adaptive_display_floor > 0.0 && st.adaptive_display_floor < 1.0)) return "adaptive_display_floor must be finite and in (0, 1)";
	if (st.denoise_dual && !st.denoise) return "denoise_dual needs denoise";
	if (st.denoise_dual && st.samples_per_iteration == 0) return "denoise_dual needs samples_per_iteration > 0 (the passes alternate between the two half buffers)";
	if (st.denoise_dual && st.denoise_features) return "denoise_dual cannot be combined with denoise_features: rmd_denoise_dual has no feature weight";
	if (st.denoise_dual_features && !st.denoise_dual) return "denoise_dual_features needs denoise_dual (it selects rmd_denoise_dual_guided)";
	if (st.denoise_dual_select && !st.denoise_dual) return "denoise_dual_select needs denoise_dual (it selects rmd_denoise_dual_select)";
	if (st.denoise_dual_atrous && !st.denoise_dual) return "denoise_dual_atrous needs denoise_dual (it selects rmd_denoise_atrous_dual)";
	if (st.denoise_dual_atrous && st.denoise_dual_select) return "denoise_dual_atrous cannot be combined with denoise_dual_select: the selection has no a-trous candidate";
	if (st.denoise_dual_atrous_region && !st.denoise_dual_atrous)
		return "denoise_dual_atrous_region needs denoise_dual_atrous (it selects rmd_denoise_atrous_dual_region for the adaptive check)";
	if (!(st.adaptive_denoised_threshold >= 0.0)) return "adaptive_denoised_threshold must be >= 0 (0 = off)";
	if (st.adaptive_denoised_threshold > 0.0 && !st.denoise_dual) return "adaptive_denoised_threshold > 0 needs denoise_dual (the error is that of the dual-buffer filter)";
	if (st.adaptive_denoised_threshold > 0.0 && st.adaptive_threshold > 0.0) return "adaptive_denoised_threshold and adaptive_threshold are mutually exclusive";
	if (st.denoise_dual && st.adaptive_measure != "channel_max") return "adaptive_measure cannot be combined with denoise_dual: the dual loop's check is rmd_tile_error_dual";
	if (st.denoise_dual && st.adaptive_display_threshold > 0.0) return "adaptive_display_threshold cannot be combined with denoise_dual: the dual loop's check is rmd_tile_error_dual";
	if (!(st.adaptive_denoised_display_threshold >= 0.0) || !std::isfinite(st.adaptive_denoised_display_threshold))
		return "adaptive_denoised_display_threshold must be finite and >= 0 (0 = off)";
	if (st.adaptive_denoised_display_threshold > 0.0 && st.samples_per_iteration == 0)
		return "adaptive_denoised_display_threshold > 0 needs samples_per_iteration > 0 (the error is checked between passes)";
	if (st.adaptive_denoised_display_threshold > 0.0 && !st.denoise_dual)
		return "adaptive_denoised_display_threshold > 0 needs denoise_dual (the error is that of the dual-buffer filter)";
	if (st.adaptive_denoised_display_threshold > 0.0 && st.adaptive_denoised_threshold > 0.0)
		return "adaptive_denoised_display_threshold and adaptive_denoised_threshold are mutually exclusive";
	if (st.adaptive_denoised_display_threshold > 0.0 && st.adaptive_threshold > 0.0)
		return "adaptive_denoised_display_threshold and adaptive_threshold are mutually exclusive";
	if (st.adaptive_display_threshold > 0.0 && st.adaptive_display_auto_exposure && st.worker_count > 1)
		return "adaptive_display_auto_exposure renders on one device: every check histograms the whole frame";
	if (st.denoise_dual && st.worker_count > 1) return "denoise_dual renders on one device: the filter's window crosses the tiles that several devices would own";
	if (!(st.denoise_feature_slope >= 0.0) || !std::isfinite(st.denoise_feature_slope)) return "denoise_feature_slope must be finite and >= 0 (0 = off)";
	if (st.denoise_feature_slope > 0.0 && (st.denoise_atrous || st.denoise_dual_atrous))
		return "denoise_feature_slope cannot be combined with denoise_atrous / denoise_dual_atrous: the a-trous filters have no slope term";
	if (st.denoise_feature_slope > 0.0 && !(st.denoise_features || st.denoise_dual_features || st.denoise_dual_select))
		return "denoise_feature_slope > 0 needs a guided non-local-means filter (denoise_features, denoise_dual_features or denoise_dual_select)";
	if (!(st.denoise_atrous_slope >= 0.0) || !std::isfinite(st.denoise_atrous_slope)) return "denoise_atrous_slope must be finite and >= 0 (0 = off)";
	if (st.denoise_atrous_slope > 0.0 && !((st.denoise_atrous && st.denoise_features) || (st.denoise_dual_atrous && st.denoise_dual_features)))
		return "denoise_atrous_slope > 0 needs a guided a-trous filter (denoise_atrous with denoise_features, or denoise_dual_atrous with denoise_dual_features)";
	if (st.despike_radius < 1 || st.despike_radius > rmd::kDespikeMaxRadius) return "despike_radius must be in [1, 3]";
	if (st.despike_rank > (2 * st.despike_radius + 1) * (2 * st.despike_radius + 1) - 2) return "despike_rank must be in [0, (2 * despike_radius + 1)^2 - 2]";
	if (!(st.despike_k >= 0.0) || !std::isfinite(st.despike_k)) return "despike_k must be finite and >= 0";
	if (!(st.despike_ratio >= 1.0) || !std::isfinite(st.despike_ratio)) return "despike_ratio must be finite and >= 1";
	if (!(st.despike_floor >= 0.0) || !std::isfinite(st.despike_floor)) return "despike_floor must be finite and >= 0";
	if (st.despike && st.denoise_dual) return "despike cannot be combined with denoise_dual: the halves are not yet despiked";
	if (st.despike && st.adaptive_threshold > 0.0 && st.worker_count > 1)
		return "despike with adaptive_threshold renders on one device: the window crosses the tiles that several devices would own";
	if (st.despike && st.adaptive_display_threshold > 0.0 && st.worker_count > 1)
		return "despike with adaptive_display_threshold renders on one device: the window crosses the tiles that several devices would own";
	if (st.despike_dual && !st.denoise_dual) return "despike_dual needs denoise_dual: it despikes the two halves"; // (after every older rule: each of their texts is still raised first)
	return "";
}
} // namespace

TaskHandle render_tiled(const Scene &scene, const Settings &settings) {
	if (const std::string why = check_settings(settings); !why.empty()) throw Error(RMD_ERR_INVALID_ARGUMENT, "render_tiled: " + why);
	TaskHandle h;
	h.settings = settings;
	h.shared_ = std::make_shared<TaskHandle::Shared>();
	const std::shared_ptr<TaskHandle::Shared> sh = h.shared_;
	if (settings.denoise_dual) {
		if (settings.denoise_dual_features || settings.denoise_dual_select) h.scene_ = std::make_shared<const Scene>(scene);
		sh->alive = 1;
		h.workers_.emplace_back([sh, scene, settings] { worker_main<DualWorker>(sh, 0, scene, settings); });
		return h;
	}
	if (settings.denoise_features) h.scene_ = std::make_shared<const Scene>(scene);
	const CameraSettings &cam = settings.camera_settings;
	for (const rmd_tile_rect &r : generate_tiles(cam.backbuffer_width, cam.backbuffer_height, settings.tile_size)) {
		Tile t;
		t.left = r.left, t.top = r.top, t.width = r.width, t.height = r.height;
		// (no data: a fresh tile's sums are the zeros of its worker's device framebuffer)
		sh->queue.push_back(std::move(t));
	}
	const size_t workers = std::max<size_t>(1, settings.worker_count);
	const size_t batch = workers == 1 ? sh->queue.size() : std::max<size_t>(1, (sh->queue.size() + workers * 4 - 1) / (workers * 4));
	sh->alive = workers;
	// worker w drives GPU w; RAYMOND_REHEARSE_ON_DEVICE0=1 (tests on a one-GPU box) gives every worker its own context on GPU 0
	const bool rehearse = std::getenv("RAYMOND_REHEARSE_ON_DEVICE0") != nullptr;
	for (size_t w = 0; w < workers; w++)
		h.workers_.emplace_back([=] { worker_main<TileWorker>(sh, rehearse ? 0 : (int)w, (int)w, workers, scene, settings, batch); });
	return h;
}

TaskHandle::~TaskHandle() {
	for (std::thread &t : workers_)
		if (t.joinable()) t.join();
}

std::vector<Vector3> TaskHandle::await() {
	const CameraSettings &cam = settings.camera_settings;
	std::vector<Vector3> out(cam.backbuffer_width * cam.backbuffer_height, Vector3{0, 0, 0});
	std::unique_lock<std::mutex> lock(shared_->m);
	shared_->cv.wait(lock, [&] { return shared_->alive == 0; }); // the reference polls every 500 ms (:88-110)
	if (!shared_->error.empty()) throw Error(RMD_ERR_HIP, shared_->error); // the reference would hang after a worker panic
	std::vector<Tile> collected; // settings.denoise
	while (!shared_->channel.empty()) {
		Message m = std::move(shared_->channel.front());
		shared_->channel.pop_front();
		if (m.kind != Message::TileFinished) break; // :101-103
		if (settings.denoise || settings.despike) collected.push_back(std::move(m.tile));
		else place_tile(m.tile, m.tile.data, cam.backbuffer_width, out, (double)m.tile.sample_count);
	}
	lock.unlock();
	if (!collected.empty() && !settings.denoise) out = despike_tiles(collected, settings, 0); // (settings.despike alone: the plain divide of the despiked sums)
	else if (!collected.empty()) out = settings.denoise_dual ? denoise_dual_tiles(collected, settings, 0, nullptr, scene_.get()) : denoise_tiles(collected, settings, 0, scene_.get()); // render_tiled's first GPU
	return out;
}

namespace {
// A first-hit pass over the rects, each at its own count, from sample 0 with the settings' seed and DOF flag: one async call per distinct non-zero
// count over the rects that share it, then synchronise.  call(scene, camera, settings, rects, n_rects) enqueues one.
template <class Call>
void first_hit_per_count(rmd_context *ctx, const Scene &scene, const Settings &st, const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts, Call call) {
	const DeviceScene dscene(ctx, scene);
	const rmd_camera cam = camera_pod(st);
	std::vector<uint32_t> distinct(counts);
	std::sort(distinct.begin(), distinct.end());
	distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
	for (uint32_t n : distinct) {
		if (n == 0) continue;
		std::vector<rmd_tile_rect> share;
		for (size_t i = 0; i < rects.size(); i++)
			if (counts[i] == n) share.push_back(rects[i]);
		const rmd_settings s = settings_pod(st, 0, n, feature_flags(st));
		call(dscene, &cam, &s, share.data(), (uint32_t)share.size());
	}
	check(rmd_context_synchronize(ctx), ctx, "rmd_context_synchronize");
}

// the feature sums of the rects into feat / feat_sq (zeroed device buffers of ctx)
void render_features_on(rmd_context *ctx, const Scene &scene, const Settings &st, const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts,
                        double *feat, double *feat_sq) {
	first_hit_per_count(ctx, scene, st, rects, counts, [&](const rmd_scene *ds, const rmd_camera *cam, const rmd_settings *s, const rmd_tile_rect *r, uint32_t n) {
		check(rmd_render_features_async(ctx, ds, cam, s, r, n, feat, feat_sq), ctx, "rmd_render_features");
	});
}
} // namespace

std::vector<double> render_features(const Scene &scene, const Settings &settings, const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts,
                                    int device, std::vector<double> *sums_sq) {
	if (rects.size() != counts.size()) throw Error(RMD_ERR_INVALID_ARGUMENT, "render_features: one sample count per rect");
	const size_t W = settings.camera_settings.backbuffer_width, H = settings.camera_settings.backbuffer_height;
	std::vector<double> out(W * H * RMD_FEATURE_CHANNELS);
	if (sums_sq) sums_sq->assign(out.size(), 0.0);
	const Context ctx(device);
	const Frame dev[2] = {Frame(ctx, W, H, Frame::Features), Frame(ctx, W, H, Frame::Features)};
	render_features_on(ctx, scene, settings, rects, counts, dev[0], sums_sq ? (double *)dev[1] : nullptr);
	check(rmd_framebuffer_download(ctx, dev[0], out.data(), out.size()), ctx, "rmd_framebuffer_download");
	if (sums_sq) check(rmd_framebuffer_download(ctx, dev[1], sums_sq->data(), sums_sq->size()), ctx, "rmd_framebuffer_download");
	return out;
}

std::vector<uint32_t> render_ids(const Scene &scene, const Settings &settings, const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts, int device) {
	if (rects.size() != counts.size()) throw Error(RMD_ERR_INVALID_ARGUMENT, "render_ids: one sample count per rect");
	const size_t W = settings.camera_settings.backbuffer_width, H = settings.camera_settings.backbuffer_height;
	std::vector<uint32_t> out(W * H * RMD_ID_WORDS);
	const Context ctx(device);
	const Frame dev(ctx, W, H, Frame::Ids);
	first_hit_per_count(ctx, scene, settings, rects, counts, [&](const rmd_scene *ds, const rmd_camera *cam, const rmd_settings *s, const rmd_tile_rect *r, uint32_t n) {
		check(rmd_render_ids_async(ctx, ds, cam, s, r, n, reinterpret_cast<uint32_t *>((double *)dev)), ctx, "rmd_render_ids");
	});
	check(rmd_framebuffer_download(ctx, dev, reinterpret_cast<double *>(out.data()), out.size() / 2), ctx, "rmd_framebuffer_download");
	return out;
}

std::vector<double> ids_matte(const std::vector<uint32_t> &words, size_t width, size_t height, const std::vector<uint32_t> &objects, int device, uint64_t *other_pixels) {
	if (words.size() != width * height * RMD_ID_WORDS) throw Error(RMD_ERR_INVALID_ARGUMENT, "ids_matte: width * height * RMD_ID_WORDS words");
	std::vector<double> out(width * height);
	const Context ctx(device);
	const Frame ids(ctx, width, height, Frame::Ids), matte(ctx, width, height);
	check(rmd_framebuffer_upload(ctx, reinterpret_cast<const double *>(words.data()), ids, words.size() / 2), ctx, "rmd_framebuffer_upload");
	check(rmd_ids_matte(ctx, reinterpret_cast<const uint32_t *>((double *)ids), (uint32_t)width, (uint32_t)height, objects.data(), (uint32_t)objects.size(), matte, other_pixels), ctx,
	      "rmd_ids_matte");
	check(rmd_framebuffer_download(ctx, matte, out.data(), out.size()), ctx, "rmd_framebuffer_download");
	return out;
}

std::vector<double> ids_matte_host(const std::vector<uint32_t> &words, size_t width, size_t height, const std::vector<uint32_t> &objects, uint64_t *other_pixels) {
	if (words.size() != width * height * RMD_ID_WORDS) throw Error(RMD_ERR_INVALID_ARGUMENT, "ids_matte_host: width * height * RMD_ID_WORDS words");
	if (objects.size() > rmd::kIdsMatteMaxObjects) throw Error(RMD_ERR_INVALID_ARGUMENT, "ids_matte_host: more than 2048 objects");
	std::vector<uint32_t> keys;
	for (uint32_t o : objects) {
		if (o == RMD_ID_MISS - 1u) throw Error(RMD_ERR_INVALID_ARGUMENT, "ids_matte_host: object index 0xFFFFFFFE: its key would be RMD_ID_MISS");
		keys.push_back(rmd::ids_key_of(o));
	}
	std::sort(keys.begin(), keys.end());
	keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
	std::vector<double> out(width * height);
	uint64_t other = 0;
	for (size_t i = 0; i < width * height; i++) {
		const uint32_t *rec = &words[i * RMD_ID_WORDS];
		out[i] = rmd::ids_matte_pixel(rec, keys.data(), (uint32_t)keys.size());
		other += rec[rmd::kIdOther] != 0u;
	}
	if (other_pixels) *other_pixels = other;
	return out;
}

std::vector<uint32_t> render_ao(const Scene &scene, const Settings &settings, const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts, double max_distance,
                                int device) {
	if (rects.size() != counts.size()) throw Error(RMD_ERR_INVALID_ARGUMENT, "render_ao: one sample count per rect");
	const size_t W = settings.camera_settings.backbuffer_width, H = settings.camera_settings.backbuffer_height;
	std::vector<uint32_t> out(W * H * RMD_AO_WORDS);
	const Context ctx(device);
	const Frame dev(ctx, W, H, Frame::Ao);
	first_hit_per_count(ctx, scene, settings, rects, counts, [&](const rmd_scene *ds, const rmd_camera *cam, const rmd_settings *s, const rmd_tile_rect *r, uint32_t n) {
		check(rmd_render_ao_async(ctx, ds, cam, s, r, n, max_distance, reinterpret_cast<uint32_t *>((double *)dev)), ctx, "rmd_render_ao");
	});
	check(rmd_framebuffer_download(ctx, dev, reinterpret_cast<double *>(out.data()), out.size() / 2), ctx, "rmd_framebuffer_download");
	return out;
}

std::vector<double> ao_resolve(const std::vector<uint32_t> &words, size_t width, size_t height, double empty_value, int device, uint64_t *empty_pixels) {
	if (words.size() != width * height * RMD_AO_WORDS) throw Error(RMD_ERR_INVALID_ARGUMENT, "ao_resolve: width * height * RMD_AO_WORDS words");
	std::vector<double> out(width * height);
	const Context ctx(device);
	const Frame ao(ctx, width, height, Frame::Ao), res(ctx, width, height);
	check(rmd_framebuffer_upload(ctx, reinterpret_cast<const double *>(words.data()), ao, words.size() / 2), ctx, "rmd_framebuffer_upload");
	check(rmd_ao_resolve(ctx, reinterpret_cast<const uint32_t *>((double *)ao), (uint32_t)width, (uint32_t)height, empty_value, res, empty_pixels), ctx, "rmd_ao_resolve");
	check(rmd_framebuffer_download(ctx, res, out.data(), out.size()), ctx, "rmd_framebuffer_download");
	return out;
}

std::vector<double> ao_resolve_host(const std::vector<uint32_t> &words, size_t width, size_t height, double empty_value, uint64_t *empty_pixels) {
	if (words.size() != width * height * RMD_AO_WORDS) throw Error(RMD_ERR_INVALID_ARGUMENT, "ao_resolve_host: width * height * RMD_AO_WORDS words");
	if (!std::isfinite(empty_value)) throw Error(RMD_ERR_INVALID_ARGUMENT, "ao_resolve_host: empty_value is not finite");
	std::vector<double> out(width * height);
	uint64_t n_empty = 0;
	for (size_t i = 0; i < width * height; i++) {
		bool empty = false;
		out[i] = rmd::ao_resolve_pixel(&words[i * RMD_AO_WORDS], empty_value, &empty);
		n_empty += empty;
	}
	if (empty_pixels) *empty_pixels = n_empty;
	return out;
}

std::vector<rmd_ray_hit> intersect_rays(const Scene &scene, const std::vector<double> &rays, int device) {
	if (rays.size() % RMD_RAY_DOUBLES != 0) throw Error(RMD_ERR_INVALID_ARGUMENT, "intersect_rays: RMD_RAY_DOUBLES doubles a ray");
	const size_t n = rays.size() / RMD_RAY_DOUBLES;
	std::vector<rmd_ray_hit> out(n);
	if (n == 0) return out;
	const Context ctx(device);
	const DeviceScene ds(ctx, scene);
	const Frame d_rays(ctx, n, 1, Frame::Rays), d_hits(ctx, n, 1, Frame::Hits);
	check(rmd_framebuffer_upload(ctx, rays.data(), d_rays, rays.size()), ctx, "rmd_framebuffer_upload");
	check(rmd_intersect_rays(ctx, ds, d_rays, n, reinterpret_cast<rmd_ray_hit *>((double *)d_hits)), ctx, "rmd_intersect_rays");
	check(rmd_framebuffer_download(ctx, d_hits, reinterpret_cast<double *>(out.data()), n * RMD_HIT_DOUBLES), ctx, "rmd_framebuffer_download");
	return out;
}

std::vector<double> camera_rays(const Settings &settings, const std::vector<uint32_t> &xy, const std::vector<double> *uv, int device) {
	if (xy.size() % 2 != 0 || (uv && uv->size() != xy.size())) throw Error(RMD_ERR_INVALID_ARGUMENT, "camera_rays: one x, y pair a ray, and one u, v pair when uv is given");
	const size_t n = xy.size() / 2;
	std::vector<double> out(n * RMD_RAY_DOUBLES);
	if (n == 0) return out;
	const rmd_camera cam = camera_pod(settings);
	const Context ctx(device);
	const Frame d_rays(ctx, n, 1, Frame::Rays);
	check(rmd_camera_rays(ctx, &cam, xy.data(), uv ? uv->data() : nullptr, n, d_rays), ctx, "rmd_camera_rays");
	check(rmd_framebuffer_download(ctx, d_rays, out.data(), out.size()), ctx, "rmd_framebuffer_download");
	return out;
}

rmd_ray_hit pick(const Scene &scene, const Settings &settings, uint32_t x, uint32_t y, int device) {
	const rmd_camera cam = camera_pod(settings);
	const uint32_t xy[2] = {x, y};
	rmd_ray_hit out;
	const Context ctx(device);
	const DeviceScene ds(ctx, scene);
	const Frame d_rays(ctx, 1, 1, Frame::Rays), d_hits(ctx, 1, 1, Frame::Hits);
	check(rmd_camera_rays(ctx, &cam, xy, nullptr, 1, d_rays), ctx, "rmd_camera_rays");
	check(rmd_intersect_rays(ctx, ds, d_rays, 1, reinterpret_cast<rmd_ray_hit *>((double *)d_hits)), ctx, "rmd_intersect_rays");
	check(rmd_framebuffer_download(ctx, d_hits, reinterpret_cast<double *>(&out), RMD_HIT_DOUBLES), ctx, "rmd_framebuffer_download");
	return out;
}

std::vector<Vector3> denoise_tiles(const std::vector<Tile> &tiles, const Settings &settings, int device, const Scene *scene, std::vector<double> *feature_means) {
	if (settings.denoise_features && !scene) throw Error(RMD_ERR_INVALID_ARGUMENT, "denoise_tiles: settings.denoise_features needs the scene");
	const size_t W = settings.camera_settings.backbuffer_width, H = settings.camera_settings.backbuffer_height;
	std::vector<Vector3> sums(W * H), sums_sq(W * H);
	std::vector<rmd_tile_rect> rects;
	std::vector<uint32_t> counts;
	for (const Tile &t : tiles) {
		if (t.data.size() != t.width * t.height || t.data_sq.size() != t.width * t.height)
			throw Error(RMD_ERR_INVALID_ARGUMENT, "denoise_tiles: a tile without its sums and sums of squares");
		place_tile(t, t.data, W, sums), place_tile(t, t.data_sq, W, sums_sq);
		rects.push_back(rect_of(t));
		counts.push_back((uint32_t)t.sample_count);
	}
	std::vector<Vector3> out(W * H);
	const Context ctx(device);
	Frame dev[3] = {Frame(ctx, W, H), Frame(ctx, W, H), Frame(ctx, W, H)};
	Frame fdev[2]; // settings.denoise_features: the feature sums and sums of squares
	if (settings.denoise_features) {
		for (Frame &f : fdev) f = Frame(ctx, W, H, Frame::Features);
		render_features_on(ctx, *scene, settings, rects, counts, fdev[0], fdev[1]);
		if (feature_means) {
			feature_means->assign(W * H * RMD_FEATURE_CHANNELS, 0.0);
			check(rmd_framebuffer_download(ctx, fdev[0], feature_means->data(), feature_means->size()), ctx, "rmd_framebuffer_download");
			divide_by_counts(*feature_means, W, H, RMD_FEATURE_CHANNELS, rects, counts);
		}
	}
	check(rmd_framebuffer_upload(ctx, reinterpret_cast<const double *>(sums.data()), dev[0], W * H * 3), ctx, "rmd_framebuffer_upload");
	check(rmd_framebuffer_upload(ctx, reinterpret_cast<const double *>(sums_sq.data()), dev[1], W * H * 3), ctx, "rmd_framebuffer_upload");
	if (settings.despike) { // before anything else: every filter below takes the despiked sums in place of the raw ones
		Frame clean[2] = {Frame(ctx, W, H), Frame(ctx, W, H)};
		check(rmd_despike(ctx, dev[0], dev[1], (uint32_t)W, (uint32_t)H, rects.data(), counts.data(), (uint32_t)rects.size(), settings.despike_radius, settings.despike_rank,
		                  settings.despike_k, settings.despike_ratio, settings.despike_floor, clean[0], clean[1], nullptr),
		      ctx, "rmd_despike");
		dev[0] = std::move(clean[0]), dev[1] = std::move(clean[1]);
	}
	if (settings.denoise_atrous && settings.denoise_features && settings.denoise_atrous_slope > 0.0)
		check(rmd_denoise_atrous_slope(ctx, dev[0], dev[1], fdev[0], fdev[1], (uint32_t)W, (uint32_t)H, rects.data(), counts.data(), (uint32_t)rects.size(),
		                               settings.denoise_atrous_levels, settings.denoise_atrous_k, settings.denoise_alpha, settings.denoise_feature_k,
		                               settings.denoise_feature_tau, settings.denoise_atrous_slope, dev[2]),
		      ctx, "rmd_denoise_atrous_slope");
	else if (settings.denoise_atrous) // (fdev both null without denoise_features: the colour weight alone)
		check(rmd_denoise_atrous(ctx, dev[0], dev[1], fdev[0], fdev[1], (uint32_t)W, (uint32_t)H, rects.data(), counts.data(), (uint32_t)rects.size(),
		                         settings.denoise_atrous_levels, settings.denoise_atrous_k, settings.denoise_alpha, settings.denoise_feature_k,
		                         settings.denoise_feature_tau, dev[2]),
		      ctx, "rmd_denoise_atrous");
	else if (settings.denoise_features && settings.denoise_feature_slope > 0.0)
		check(rmd_denoise_guided_slope(ctx, dev[0], dev[1], fdev[0], fdev[1], (uint32_t)W, (uint32_t)H, rects.data(), counts.data(), (uint32_t)rects.size(),
		                               settings.denoise_radius, settings.denoise_patch, settings.denoise_k, settings.denoise_alpha, settings.denoise_feature_k,
		                               settings.denoise_feature_tau, settings.denoise_feature_slope, dev[2]),
		      ctx, "rmd_denoise_guided_slope");
	else // (fdev both null without denoise_features: exactly rmd_denoise)
		check(rmd_denoise_guided(ctx, dev[0], dev[1], fdev[0], fdev[1], (uint32_t)W, (uint32_t)H, rects.data(), counts.data(), (uint32_t)rects.size(),
		                         settings.denoise_radius, settings.denoise_patch, settings.denoise_k, settings.denoise_alpha, settings.denoise_feature_k,
		                         settings.denoise_feature_tau, dev[2]),
		      ctx, "rmd_denoise_guided");
	check(rmd_framebuffer_download(ctx, dev[2], reinterpret_cast<double *>(out.data()), W * H * 3), ctx, "rmd_framebuffer_download");
	return out;
}

std::vector<Vector3> despike_tiles(const std::vector<Tile> &tiles, const Settings &settings, int device) {
	const size_t W = settings.camera_settings.backbuffer_width, H = settings.camera_settings.backbuffer_height;
	std::vector<Vector3> sums(W * H), sums_sq(W * H);
	std::vector<rmd_tile_rect> rects;
	std::vector<uint32_t> counts;
	for (const Tile &t : tiles) {
		if (t.data.size() != t.width * t.height || t.data_sq.size() != t.width * t.height)
			throw Error(RMD_ERR_INVALID_ARGUMENT, "despike_tiles: a tile without its sums and sums of squares");
		place_tile(t, t.data, W, sums), place_tile(t, t.data_sq, W, sums_sq);
		rects.push_back(rect_of(t));
		counts.push_back((uint32_t)t.sample_count);
	}
	const Context ctx(device);
	const Frame dev[4] = {Frame(ctx, W, H), Frame(ctx, W, H), Frame(ctx, W, H), Frame(ctx, W, H)};
	check(rmd_framebuffer_upload(ctx, reinterpret_cast<const double *>(sums.data()), dev[0], W * H * 3), ctx, "rmd_framebuffer_upload");
	check(rmd_framebuffer_upload(ctx, reinterpret_cast<const double *>(sums_sq.data()), dev[1], W * H * 3), ctx, "rmd_framebuffer_upload");
	check(rmd_despike(ctx, dev[0], dev[1], (uint32_t)W, (uint32_t)H, rects.data(), counts.data(), (uint32_t)rects.size(), settings.despike_radius, settings.despike_rank,
	                  settings.despike_k, settings.despike_ratio, settings.despike_floor, dev[2], dev[3], nullptr),
	      ctx, "rmd_despike");
	check(rmd_framebuffer_download(ctx, dev[2], reinterpret_cast<double *>(sums.data()), W * H * 3), ctx, "rmd_framebuffer_download");
	// the plain divide (:93-99): every tile's pixels by its own count; a pixel no finished tile covers stays 0
	std::vector<Vector3> out(W * H, Vector3{0, 0, 0});
	for (const Tile &t : tiles)
		for (size_t y = 0; y < t.height; y++)
			for (size_t x = 0; x < t.width; x++) {
				const size_t at = (t.top + y) * W + t.left + x;
				for (int c = 0; c < 3; c++) out[at][c] = sums[at][c] / (double)t.sample_count;
			}
	return out;
}

std::vector<uint32_t> despike_host(const std::vector<Vector3> &sums, const std::vector<Vector3> &sums_sq, size_t width, size_t height, const std::vector<rmd_tile_rect> &rects,
                                   const std::vector<uint32_t> &counts, uint32_t radius, uint32_t rank, double k, double ratio, double floor,
                                   std::vector<Vector3> &out_sums, std::vector<Vector3> &out_sums_sq) {
	if (sums.size() != width * height || sums_sq.size() != width * height || rects.size() != counts.size() || radius < 1 || radius > rmd::kDespikeMaxRadius)
		throw Error(RMD_ERR_INVALID_ARGUMENT, "despike_host: bad argument");
	const size_t r = radius, AW = width + 2 * r, AH = height + 2 * r;
	std::vector<uint32_t> n(width * height, 0u), rect_of_pixel(width * height, 0u), replaced(rects.size(), 0u);
	for (size_t j = 0; j < rects.size(); j++)
		for (size_t y = rects[j].top; y < (size_t)rects[j].top + rects[j].height; y++)
			for (size_t x = rects[j].left; x < (size_t)rects[j].left + rects[j].width; x++) n[y * width + x] = counts[j], rect_of_pixel[y * width + x] = (uint32_t)j;
	// the kernel's apron, for the whole frame at once: Y and V, a NaN Y where there is no other
	std::vector<double> Y(AW * AH, std::nan("")), V(AW * AH, 0.0);
	for (size_t y = 0; y < height; y++)
		for (size_t x = 0; x < width; x++) {
			double yy, vv;
			if (rmd::despike_pixel(sums[y * width + x].data(), sums_sq[y * width + x].data(), n[y * width + x], yy, vv)) Y[(y + r) * AW + x + r] = yy, V[(y + r) * AW + x + r] = vv;
		}
	out_sums = sums, out_sums_sq = sums_sq;
	const int side = 2 * (int)radius + 1;
	for (size_t y = 0; y < height; y++)
		for (size_t x = 0; x < width; x++) {
			const size_t centre = (y + r) * AW + x + r, p = y * width + x;
			const double yp = Y[centre];
			const double *win = Y.data() + (centre - r * AW - r);
			if (!(yp == yp) || rmd::despike_settled(rmd::despike_at_or_above(win, (uint32_t)AW, radius, yp), rank, yp)) continue;
			const int donor = rmd::despike_donor(win, (uint32_t)AW, radius, rank);
			if (donor < 0) continue;
			const int dy = donor / side - (int)radius, dx = donor % side - (int)radius;
			const size_t at = (size_t)((int64_t)centre + dy * (int64_t)AW + dx), q = (size_t)((int64_t)p + dy * (int64_t)width + dx);
			if (!rmd::despike_is_spike(yp, Y[at], V[at], k, ratio, floor)) continue;
			replaced[rect_of_pixel[p]]++;
			for (int c = 0; c < 3; c++) {
				out_sums[p][c] = n[p] == n[q] ? sums[q][c] : rmd::despike_scaled(sums[q][c], n[q], n[p]);
				out_sums_sq[p][c] = n[p] == n[q] ? sums_sq[q][c] : rmd::despike_scaled(sums_sq[q][c], n[q], n[p]);
			}
		}
	return replaced;
}

std::vector<uint32_t> despike_dual_host(const std::vector<Vector3> &sums_a, const std::vector<Vector3> &sums_sq_a, const std::vector<Vector3> &sums_b,
                                        const std::vector<Vector3> &sums_sq_b, size_t width, size_t height, const std::vector<rmd_tile_rect> &rects,
                                        const std::vector<uint32_t> &counts_a, const std::vector<uint32_t> &counts_b, uint32_t radius, uint32_t rank, double k, double ratio,
                                        double floor, std::vector<Vector3> &out_a, std::vector<Vector3> &out_sq_a, std::vector<Vector3> &out_b, std::vector<Vector3> &out_sq_b) {
	const size_t N = width * height;
	bool bad = sums_a.size() != N || sums_sq_a.size() != N || sums_b.size() != N || sums_sq_b.size() != N || rects.size() != counts_a.size() || rects.size() != counts_b.size() ||
	           radius < 1 || radius > rmd::kDespikeMaxRadius;
	for (size_t j = 0; !bad && j < rects.size(); j++) bad = (uint64_t)counts_a[j] + counts_b[j] > 0xFFFFFFFFull;
	if (bad) throw Error(RMD_ERR_INVALID_ARGUMENT, "despike_dual_host: bad argument");
	const size_t r = radius, AW = width + 2 * r, AH = height + 2 * r;
	std::vector<uint32_t> na(N, 0u), nb(N, 0u), rect_of_pixel(N, 0u), replaced(rects.size(), 0u);
	for (size_t j = 0; j < rects.size(); j++)
		for (size_t y = rects[j].top; y < (size_t)rects[j].top + rects[j].height; y++)
			for (size_t x = rects[j].left; x < (size_t)rects[j].left + rects[j].width; x++)
				na[y * width + x] = counts_a[j], nb[y * width + x] = counts_b[j], rect_of_pixel[y * width + x] = (uint32_t)j;
	// the kernel's apron, for the whole frame at once: Y and V of the merged pixel, a NaN Y where there is no other
	std::vector<double> Y(AW * AH, std::nan("")), V(AW * AH, 0.0);
	for (size_t y = 0; y < height; y++)
		for (size_t x = 0; x < width; x++) {
			const size_t p = y * width + x;
			double yy, vv;
			if (rmd::despike_dual_pixel(sums_a[p].data(), sums_sq_a[p].data(), na[p], sums_b[p].data(), sums_sq_b[p].data(), nb[p], yy, vv))
				Y[(y + r) * AW + x + r] = yy, V[(y + r) * AW + x + r] = vv;
		}
	out_a = sums_a, out_sq_a = sums_sq_a, out_b = sums_b, out_sq_b = sums_sq_b;
	const int side = 2 * (int)radius + 1;
	for (size_t y = 0; y < height; y++)
		for (size_t x = 0; x < width; x++) {
			const size_t centre = (y + r) * AW + x + r, p = y * width + x;
			const double yp = Y[centre];
			const double *win = Y.data() + (centre - r * AW - r);
			if (!(yp == yp) || rmd::despike_settled(rmd::despike_at_or_above(win, (uint32_t)AW, radius, yp), rank, yp)) continue;
			const int donor = rmd::despike_donor(win, (uint32_t)AW, radius, rank);
			if (donor < 0) continue;
			const int dy = donor / side - (int)radius, dx = donor % side - (int)radius;
			const size_t at = (size_t)((int64_t)centre + dy * (int64_t)AW + dx), q = (size_t)((int64_t)p + dy * (int64_t)width + dx);
			if (!rmd::despike_is_spike(yp, Y[at], V[at], k, ratio, floor)) continue;
			replaced[rect_of_pixel[p]]++;
			for (int c = 0; c < 3; c++) {
				out_a[p][c] = rmd::despike_dual_take(sums_a[q][c], na[q], na[p]), out_sq_a[p][c] = rmd::despike_dual_take(sums_sq_a[q][c], na[q], na[p]);
				out_b[p][c] = rmd::despike_dual_take(sums_b[q][c], nb[q], nb[p]), out_sq_b[p][c] = rmd::despike_dual_take(sums_sq_b[q][c], nb[q], nb[p]);
			}
		}
	return replaced;
}

// tile_luma_error_host and tile_weighted_error_host: the checks, then each rect through the rule's tile_*_rect_host.  measure(S, Q, rect, count): the rule's result
template <class Result, class Measure>
static std::vector<Result> tile_measure_host(const std::string &name, const std::vector<Vector3> &sums, const std::vector<Vector3> &sums_sq, size_t width, size_t height,
                                             const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts, bool bad_parameter, Measure measure) {
	if (sums.size() != width * height || sums_sq.size() != width * height || rects.size() != counts.size() || bad_parameter) throw Error(RMD_ERR_INVALID_ARGUMENT, name + ": bad argument");
	std::vector<Result> out(rects.size());
	const double *S = sums.empty() ? nullptr : sums[0].data(), *Q = sums_sq.empty() ? nullptr : sums_sq[0].data();
	for (size_t j = 0; j < rects.size(); j++) {
		const rmd_tile_rect &r = rects[j];
		if ((size_t)r.left + r.width > width || (size_t)r.top + r.height > height) throw Error(RMD_ERR_INVALID_ARGUMENT, name + ": tile rectangle outside the framebuffer");
		out[j] = measure(S, Q, r, counts[j]);
	}
	return out;
}

std::vector<rmd_tile_luma> tile_luma_error_host(const std::vector<Vector3> &sums, const std::vector<Vector3> &sums_sq, size_t width, size_t height,
                                                const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts, double floor) {
	const auto measure = [&](const double *S, const double *Q, const rmd_tile_rect &r, uint32_t n) {
		const rmd::TileLuma t = rmd::tile_luma_rect_host(S, Q, (uint32_t)width, r.left, r.top, r.width, r.height, n, floor);
		return rmd_tile_luma{t.tile_rms, t.pixel_rms, t.mean_luma, t.mean_variance, t.mean_rel_variance, t.valid, t.invalid};
	};
	return tile_measure_host<rmd_tile_luma>("tile_luma_error_host", sums, sums_sq, width, height, rects, counts, false, measure);
}

std::vector<rmd_tile_weighted> tile_weighted_error_host(const std::vector<Vector3> &sums, const std::vector<Vector3> &sums_sq, size_t width, size_t height,
                                                        const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts, const std::vector<double> &weights) {
	const auto measure = [&](const double *S, const double *Q, const rmd_tile_rect &r, uint32_t n) {
		const rmd::TileWeighted t = rmd::tile_weighted_rect_host(S, Q, (uint32_t)width, r.left, r.top, r.width, r.height, n, weights.data());
		return rmd_tile_weighted{t.rms, t.mean_weighted_variance, t.mean_luma, t.mean_variance, t.valid, t.invalid};
	};
	return tile_measure_host<rmd_tile_weighted>("tile_weighted_error_host", sums, sums_sq, width, height, rects, counts, weights.size() != RMD_LUMA_WEIGHTS, measure);
}

std::vector<rmd_tile_weighted> tile_weighted_error_dual_host(const std::vector<Vector3> &out, const std::vector<double> &err, size_t width, size_t height,
                                                             const std::vector<rmd_tile_rect> &rects, const std::vector<double> &weights) {
	const std::string name = "tile_weighted_error_dual_host";
	if (out.size() != width * height || err.size() != width * height || weights.size() != RMD_LUMA_WEIGHTS) throw Error(RMD_ERR_INVALID_ARGUMENT, name + ": bad argument");
	std::vector<rmd_tile_weighted> result(rects.size());
	const double *O = out.empty() ? nullptr : out[0].data();
	for (size_t j = 0; j < rects.size(); j++) {
		const rmd_tile_rect &r = rects[j];
		if ((size_t)r.left + r.width > width || (size_t)r.top + r.height > height) throw Error(RMD_ERR_INVALID_ARGUMENT, name + ": tile rectangle outside the framebuffer");
		const rmd::TileWeighted t = rmd::tile_weighted_dual_rect_host(O, err.data(), (uint32_t)width, r.left, r.top, r.width, r.height, weights.data());
		result[j] = rmd_tile_weighted{t.rms, t.mean_weighted_variance, t.mean_luma, t.mean_variance, t.valid, t.invalid};
	}
	return result;
}

std::vector<double> display_weights(double exposure, double gamma, double display_floor) {
	std::vector<double> weights(RMD_LUMA_WEIGHTS);
	check(rmd_display_weights(exposure, gamma, display_floor, weights.data()), nullptr, "rmd_display_weights");
	return weights;
}

std::vector<Vector3> denoise_dual_tiles(const std::vector<Tile> &tiles, const Settings &settings, int device, std::vector<double> *tile_errors, const Scene *scene) {
	if (settings.denoise_dual_features && !scene) throw Error(RMD_ERR_INVALID_ARGUMENT, "denoise_dual_tiles: settings.denoise_dual_features needs the scene");
	if (settings.denoise_dual_select && !scene) throw Error(RMD_ERR_INVALID_ARGUMENT, "denoise_dual_tiles: settings.denoise_dual_select needs the scene");
	const size_t W = settings.camera_settings.backbuffer_width, H = settings.camera_settings.backbuffer_height;
	std::vector<Vector3> halves[4];
	for (std::vector<Vector3> &h : halves) h.resize(W * H);
	std::vector<rmd_tile_rect> rects;
	std::vector<uint32_t> counts_a, counts_b;
	for (const Tile &t : tiles) {
		const TileData *src[4] = {&t.data_a, &t.data_sq_a, &t.data_b, &t.data_sq_b};
		for (int i = 0; i < 4; i++) {
			if (src[i]->size() != t.width * t.height) throw Error(RMD_ERR_INVALID_ARGUMENT, "denoise_dual_tiles: a tile without its two halves' sums and sums of squares");
			place_tile(t, *src[i], W, halves[i]);
		}
		rects.push_back(rect_of(t));
		counts_a.push_back((uint32_t)t.count_a), counts_b.push_back((uint32_t)t.count_b);
	}
	std::vector<Vector3> out(W * H);
	const Context ctx(device);
	const Frame dev[6] = {Frame(ctx, W, H), Frame(ctx, W, H), Frame(ctx, W, H), Frame(ctx, W, H), Frame(ctx, W, H), Frame(ctx, W, H)}; // the four halves, the frame, the error image
	for (int i = 0; i < 4; i++) check(rmd_framebuffer_upload(ctx, reinterpret_cast<const double *>(halves[i].data()), dev[i], W * H * 3), ctx, "rmd_framebuffer_upload");
	Frame fdev[2]; // the feature sums and sums of squares, each tile at count_a + count_b: for the guided filter, the selecting one, and the fast one when it is guided
	if (settings.denoise_dual_features || (settings.denoise_dual_select && !settings.denoise_dual_atrous)) {
		for (Frame &f : fdev) f = Frame(ctx, W, H, Frame::Features);
		render_features_on(ctx, *scene, settings, rects, sum_counts(counts_a, counts_b), fdev[0], fdev[1]);
	}
	Frame clean[4]; // settings.despike_dual: before anything else, the filter takes the despiked halves in place of the raw ones
	if (settings.despike_dual) {
		for (Frame &f : clean) f = Frame(ctx, W, H);
		check(rmd_despike_dual(ctx, dev[0], dev[1], dev[2], dev[3], (uint32_t)W, (uint32_t)H, rects.data(), counts_a.data(), counts_b.data(), (uint32_t)rects.size(),
		                       settings.despike_radius, settings.despike_rank, settings.despike_k, settings.despike_ratio, settings.despike_floor, clean[0], clean[1], clean[2],
		                       clean[3], nullptr),
		      ctx, "rmd_despike_dual");
	}
	denoise_dual_frame(ctx, settings, W, H, settings.despike_dual ? clean : dev, fdev[0], fdev[1], rects, counts_a, counts_b, nullptr, 0, dev[4],
	                   tile_errors ? (double *)dev[5] : nullptr);
	if (tile_errors) {
		tile_errors->assign(rects.size(), 0.0);
		check(rmd_tile_error_dual(ctx, dev[5], (uint32_t)W, (uint32_t)H, rects.data(), (uint32_t)rects.size(), tile_errors->data()), ctx, "rmd_tile_error_dual");
	}
	check(rmd_framebuffer_download(ctx, dev[4], reinterpret_cast<double *>(out.data()), W * H * 3), ctx, "rmd_framebuffer_download");
	return out;
}

double TaskHandle::setup_seconds() const {
	std::lock_guard<std::mutex> lock(shared_->m);
	return shared_->setup_s;
}

bool TaskHandle::finished() const {
	std::lock_guard<std::mutex> lock(shared_->m);
	return shared_->alive == 0;
}

std::optional<Message> TaskHandle::poll() {
	std::lock_guard<std::mutex> lock(shared_->m);
	if (shared_->channel.empty()) return std::nullopt;
	Message m = std::move(shared_->channel.front());
	shared_->channel.pop_front();
	return m;
}

void TaskHandle::async_await() {
	for (;;) {
		std::optional<Message> m;
		{
			std::lock_guard<std::mutex> lock(shared_->m);
			if (shared_->channel.empty() || shared_->channel.front().kind == Message::TileFinished) return;
			m = std::move(shared_->channel.front());
			shared_->channel.pop_front();
		}
		if (m->kind == Message::FramePreview) {
			if (preview_callback_) preview_callback_(*m->preview);
		} else if (callback_) callback_(m->tile);
	}
}

// ---------------------------------------------------------------- output stage (cli_old/src/main.rs:155-197)
std::vector<uint8_t> resolve_tonemap_tiles(rmd_context *ctx, const double *accum_dev, const double *accum2_dev, size_t width, size_t height,
                                           const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts, double exposure, double gamma) {
	if (counts.size() != rects.size()) throw Error(RMD_ERR_INVALID_ARGUMENT, "resolve_tonemap_tiles: one sample count per rect");
	std::vector<uint8_t> packed(pixels_of(rects) * 3);
	check(rmd_resolve_tonemap_tiles(ctx, accum_dev, accum2_dev, (uint32_t)width, (uint32_t)height, rects.data(), counts.data(), (uint32_t)rects.size(), exposure, gamma,
	                                packed.data()),
	      ctx, "rmd_resolve_tonemap_tiles");
	return packed;
}

void scatter_tiles(const std::vector<rmd_tile_rect> &rects, const std::vector<uint8_t> &packed, size_t width, size_t height, std::vector<uint8_t> &frame) {
	scatter_packed(rects, packed.data(), packed.size(), width, height, frame);
}

rmd_luma_histogram luminance_histogram(const std::vector<Vector3> &image) {
	static_assert(sizeof(rmd_luma_histogram) == (rmd::kLumaCounters + 1) * 8 && offsetof(rmd_luma_histogram, below) == rmd::kLumaBelow * 8 &&
	              offsetof(rmd_luma_histogram, not_finite) == rmd::kLumaNotFinite * 8 && offsetof(rmd_luma_histogram, pixels) == rmd::kLumaCounters * 8,
	              "luma_bins.hpp's counters are the struct's fields in order");
	uint64_t counters[rmd::kLumaCounters + 1] = {};
	for (const Vector3 &p : image) counters[rmd::luma_counter(rmd::luma_bits(rmd::luma_of(p[0], p[1], p[2])))]++; // (means: a count of 1)
	counters[rmd::kLumaCounters] = image.size();
	rmd_luma_histogram h;
	std::memcpy(&h, counters, sizeof(h));
	return h;
}

std::vector<uint8_t> tone_map(const std::vector<Vector3> &image, double exposure, double gamma) {
	std::vector<uint8_t> out(image.size() * 3, 0);
	for (size_t i = 0; i < image.size(); i++) {
		double v[3];
		bool ok = true;
		for (int c = 0; c < 3; c++) {
			double tm = 1.0 - std::exp(image[i][c] * -1.0 * exposure);
			tm = std::pow(tm, 1.0 / gamma);
			v[c] = tm * 255.0;
			ok = ok && v[c] > -1.0 && v[c] < 256.0;
		}
		if (ok)
			for (int c = 0; c < 3; c++) out[i * 3 + c] = (uint8_t)v[c];
	}
	return out;
}

void write_ppm(const std::string &path, const std::vector<uint8_t> &rgb8, size_t width, size_t height) {
	std::ofstream f(path, std::ios::binary);
	f << "P6\n" << width << " " << height << "\n255\n";
	f.write(reinterpret_cast<const char *>(rgb8.data()), (std::streamsize)rgb8.size());
}

// ---------------------------------------------------------------- benchmark inputs (mirror of raymond_amd/scenes.py)
namespace {
void room_planes(Scene &s) { // cli_old/src/main.rs:77-127
	s.objects.push_back({Geometry::Plane_({{0, -1, 0}, {0, 1, 0}}), Material::Diffuse({0.75, 0.75, 0.75}, 0.5)});
	s.objects.push_back({Geometry::Plane_({{0, 2, 0}, {0, -1, 0}}), Material::Emission({1.5, 1.5, 1.5}, {1, 1, 1}, 0.27, 0.0)});
	s.objects.push_back({Geometry::Plane_({{0, 0, -2}, {0, 0, 1}}), Material::Diffuse({1, 1, 1}, 0.4)});
	s.objects.push_back({Geometry::Plane_({{0, 0, 5}, {0, 0, -1}}), Material::Diffuse({0, 0, 0}, 0.9)});
	s.objects.push_back({Geometry::Plane_({{-2, 0, 0}, {1, 0, 0}}), Material::Diffuse({0, 0, 0}, 0.3)});
	s.objects.push_back({Geometry::Plane_({{2, 0, 0}, {-1, 0, 0}}), Material::Diffuse({0, 0, 0}, 0.3)});
}
} // namespace

Scene reflective_spheres() {
	Scene s;
	s.objects.push_back({Geometry::Sphere_({{-1.0, -0.5, 3.5}, 0.5}), Material::Diffuse({1.0, 0.0, 0.0}, 0.02)});
	s.objects.push_back({Geometry::Sphere_({{0.74, -0.25, 3.5}, 0.75}), Material::Metal({0.05, 0.25, 1.0}, 0.01)});
	room_planes(s);
	return s;
}

// Same arithmetic, in the same order, as raymond_amd.scenes.lumpy_sphere_mesh (IEEE-exact operations only),
// so both produce bit-identical triangles.
Mesh lumpy_sphere_mesh(int n, Vector3 extent, Vector3 centre) {
	std::map<std::tuple<int, int, int>, int> index;
	std::vector<std::array<int, 3>> lattice;
	auto vid = [&](int i, int j, int k) {
		auto key = std::make_tuple(i, j, k);
		auto it = index.find(key);
		if (it != index.end()) return it->second;
		int v = (int)lattice.size();
		index.emplace(key, v);
		lattice.push_back({i, j, k});
		return v;
	};
	std::vector<std::array<int, 3>> faces;
	const int spec[6][4] = {{0, n, 1, 2}, {0, 0, 2, 1}, {1, n, 2, 0}, {1, 0, 0, 2}, {2, n, 0, 1}, {2, 0, 1, 0}};
	for (const auto &f : spec)
		for (int a = 0; a < n; a++)
			for (int b = 0; b < n; b++) {
				auto p = [&](int da, int db) {
					int c[3] = {0, 0, 0};
					c[f[0]] = f[1], c[f[2]] = a + da, c[f[3]] = b + db;
					return vid(c[0], c[1], c[2]);
				};
				int v00 = p(0, 0), v10 = p(1, 0), v11 = p(1, 1), v01 = p(0, 1);
				faces.push_back({v00, v10, v11});
				faces.push_back({v00, v11, v01});
			}
	const size_t nv = lattice.size();
	std::vector<Vector3> p(nv);
	auto t3 = [](double t) { return (4.0 * t * t - 3.0) * t; };
	auto t2 = [](double t) { return 2.0 * t * t - 1.0; };
	const double step = 2.0 / n;
	Vector3 half{0, 0, 0};
	for (size_t i = 0; i < nv; i++) {
		double c[3], d[3];
		for (int a = 0; a < 3; a++) c[a] = (double)lattice[i][a] * step - 1.0;
		double len = std::sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
		for (int a = 0; a < 3; a++) d[a] = c[a] / len;
		double radius = 1.0 + 0.22 * t3(d[0]) * t3(d[1]) + 0.15 * t2(d[2]) * t3(d[1]) + 0.10 * t3(d[2]) * t2(d[0]);
		for (int a = 0; a < 3; a++) {
			p[i][a] = d[a] * radius;
			half[a] = std::max(half[a], std::fabs(p[i][a]));
		}
	}
	Vector3 scale;
	for (int a = 0; a < 3; a++) scale[a] = extent[a] * 0.5 / half[a];
	for (size_t i = 0; i < nv; i++)
		for (int a = 0; a < 3; a++) p[i][a] = p[i][a] * scale[a] + centre[a];
	std::vector<Vector3> fn(faces.size()), vn(nv, Vector3{0, 0, 0});
	for (size_t f = 0; f < faces.size(); f++) {
		const Vector3 &p0 = p[faces[f][0]], &p1 = p[faces[f][1]], &p2 = p[faces[f][2]];
		double e1[3], e2[3];
		for (int a = 0; a < 3; a++) e1[a] = p1[a] - p0[a], e2[a] = p2[a] - p0[a];
		fn[f] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
	}
	for (int k = 0; k < 3; k++) // np.add.at(vn, faces[:, k], fn): sequential, corner by corner
		for (size_t f = 0; f < faces.size(); f++)
			for (int a = 0; a < 3; a++) vn[faces[f][k]][a] += fn[f][a];
	for (size_t i = 0; i < nv; i++) {
		double len = std::sqrt((vn[i][0] * vn[i][0] + vn[i][1] * vn[i][1]) + vn[i][2] * vn[i][2]);
		for (int a = 0; a < 3; a++) vn[i][a] = vn[i][a] / len;
	}
	Mesh m;
	m.tri_pos.reserve(faces.size() * 9), m.tri_nrm.reserve(faces.size() * 9);
	for (const auto &f : faces) {
		for (int k = 0; k < 3; k++)
			for (int a = 0; a < 3; a++) m.tri_pos.push_back(p[f[k]][a]);
		for (int k = 0; k < 3; k++)
			for (int a = 0; a < 3; a++) m.tri_nrm.push_back(vn[f[k]][a]);
	}
	return m;
}

Scene gold_dragon_standin(int n) {
	Mesh mesh = lumpy_sphere_mesh(n);
	mesh.bake_transform({0.0, -0.3, 2.9}); // cli_old/src/main.rs:61
	Scene s;
	s.objects.push_back({Geometry::Sphere_({{-1.0, -0.5, 3.5}, 0.5}), Material::Diffuse({1.0, 0.0, 0.0}, 0.02)});
	s.objects.push_back({Geometry::Grid(AccGrid::build_from_mesh(mesh)), Material::Metal({1.0, 1.0, 0.1}, 0.15)}); // :63,:72-75
	room_planes(s);
	return s;
}

} // namespace raymond
