// raymond.hpp — C++ host mirror of the reference's public API above the hot path, over the C-ABI.
//
// The reference's Rust crates keep their Scene/Camera/Material API and their tile scheduler; only the per-tile
// body (src/trace.rs:197-205) moves to the GPU.  No Rust toolchain exists in this image, so the host side is
// written in C++ with the reference's names, argument meaning and call sequence:
//
//     Scene scene;  scene.objects.push_back(Object{Geometry::Sphere(...), Material::Diffuse(...)});      core/src/scene.rs
//     Mesh mesh = Mesh::load_ply(path);  mesh.bake_transform({0,-0.3,2.9});                               core/src/geometry/mesh.rs:48-121
//     auto grid = AccGrid::build_from_mesh(mesh);                                                         core/src/geometry/acc_grid.rs:36
//     Settings settings{...};  TaskHandle h = render_tiled(scene, settings);  auto image = h.await();     src/trace.rs:137, :82
//
// What differs: a worker is a GPU (an rmd_context) instead of an OS thread, and a worker's unit of work is
// "samples_per_iteration samples for a batch of tiles" in one rmd_render_tiles call instead of one sample of one
// tile.  A tile's running sums stay RESIDENT in its worker's device framebuffer between passes; what crosses the bus is what a
// message carries — a pass's TileProgressed snapshots, the TileFinished tiles — downloaded in Tile.data layout on a copy stream
// while the next pass renders.  Failures throw raymond::Error (the reference panics).
#pragma once
#include <array>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/raymond_hip.h"

namespace raymond {

using Vector3 = std::array<double, 3>; // cgmath::Vector3<f64> (core/src/lib.rs:5)

struct Error : std::runtime_error {
	rmd_status status;
	Error(rmd_status s, const std::string &what) : std::runtime_error(what), status(s) {}
};

// core/src/lib.rs:21-26
struct Material {
	uint32_t kind;
	Vector3 color;
	double roughness;
	std::array<double, 5> aux;
	static Material Diffuse(Vector3 color, double roughness) { return {RMD_MAT_DIFFUSE, color, roughness, {}}; }
	static Material Metal(Vector3 color, double roughness) { return {RMD_MAT_METAL, color, roughness, {}}; }
	static Material Emission(Vector3 e, Vector3 v2 = {1, 1, 1}, double f1 = 0, double f2 = 0) {
		return {RMD_MAT_EMISSION, e, 0.0, {v2[0], v2[1], v2[2], f1, f2}};
	}
};

struct Plane { // core/src/geometry/primitives/plane.rs:5-8
	Vector3 origin, normal;
};
struct Sphere { // core/src/geometry/primitives/sphere.rs:5-8
	Vector3 origin;
	double radius;
};

// core/src/geometry/mesh.rs:10-13 — triangles as 9 doubles of positions + 9 of vertex normals
struct Mesh {
	std::vector<double> tri_pos, tri_nrm;
	size_t triangle_count() const { return tri_pos.size() / 9; }
	// mesh.rs:58-121: ASCII PLY; only `element vertex N` is read from the header, vertex lines are
	// `x y z nx ny nz [s t]`, face lines `3 i j k`; faces with another vertex count are dropped.
	static Mesh load_ply(const std::string &path);
	// mesh.rs:48-56
	void bake_transform(Vector3 translate);
};

// core/src/geometry/acc_grid.rs:27-33 (compact layout of rmd_grid_desc); owns its arrays
class AccGrid {
  public:
	static std::shared_ptr<AccGrid> build_from_mesh(const Mesh &mesh); // acc_grid.rs:36-83 via rmd_grid_build_from_mesh
	~AccGrid();
	const rmd_grid_desc &desc() const { return desc_; }

  private:
	AccGrid() = default;
	rmd_grid_build *build_ = nullptr;
	rmd_grid_desc desc_{};
};

// core/src/scene.rs:9-13
struct Geometry {
	uint32_t kind;
	Plane plane{};
	Sphere sphere{};
	std::shared_ptr<AccGrid> grid; // Arc<AccGrid>
	static Geometry Plane_(Plane p) { return {RMD_GEOM_PLANE, p, {}, nullptr}; }
	static Geometry Sphere_(Sphere s) { return {RMD_GEOM_SPHERE, {}, s, nullptr}; }
	static Geometry Grid(std::shared_ptr<AccGrid> g) { return {RMD_GEOM_GRID, {}, {}, std::move(g)}; }
};
struct Object { // core/src/scene.rs:33-37
	Geometry geometry;
	Material material;
};
struct Scene { // core/src/scene.rs:42-52
	std::vector<Object> objects;
};

struct Transform { // src/transform.rs:4-14
	Vector3 position{0, 0, 0};
	static Transform identity() { return {}; }
};
struct CameraSettings { // src/trace.rs:32-40
	size_t backbuffer_width = 0, backbuffer_height = 0;
	double fov_vert = 55.0;
	Transform transform;
	double focal_length = 2.5, aperture_radius = 0.0;
};
struct Settings { // src/trace.rs:42-55 (+ the RNG seed the reference lacks)
	size_t worker_count = 1; // number of GPUs (the reference: num_cpus::get() threads)
	CameraSettings camera_settings;
	size_t sample_count = 1;
	size_t samples_per_iteration = 0;
	std::pair<size_t, size_t> tile_size{32, 32};
	size_t bounce_limit = 5;
	uint64_t seed = 0x5EED0001ull;
	bool use_dof = false; // opt-in: generate_primary_ray_with_dof (src/trace.rs:335-360); the reference's loop never calls it (:199)
	// opt-in (raymond_hip.h: RMD_RENDER_END_BLACK_PATHS): end zero-throughput paths in scenes with meshes too; false = reference-identical
	bool end_black_paths = false;
	// Adaptive tile sampling (an extension; 0 = off, the reference's behaviour): after every progressive pass a tile whose relative standard error
	// (raymond_hip.h: rmd_tile_error, floor `adaptive_floor`) is at most `adaptive_threshold` is finished at the samples it has.  Needs
	// samples_per_iteration > 0; render_tiled throws raymond::Error otherwise, and for a negative threshold.
	double adaptive_threshold = 0.0;
	double adaptive_floor = 1e-3;
	// What that check compares with the threshold: "channel_max", rmd_tile_error — the worst channel of the worst pixel —, or one rmd_tile_luma_error call's
	// tile_rms ("luma_tile": the RMS standard error of the tile's luminance over the tile's mean luminance) or pixel_rms ("luma_pixel": the RMS of the pixels'
	// relative luminance errors), both at `adaptive_floor`; a finished tile's `error` is then that value.  The three thresholds are not comparable numbers.
	// render_tiled throws for any other value whether or not adaptive sampling is on, and for a luma measure with denoise_dual, whose check is its own.
	std::string adaptive_measure = "channel_max";
	// Adaptive sampling by the DISPLAYED error (an extension; 0 = off; in place of adaptive_threshold, needs samples_per_iteration > 0): the check is one
	// rmd_tile_weighted_error call over the live tiles under rmd_display_weights' table — every pixel's luminance variance times the squared slope of the tone
	// curve (1 - exp(-y exposure))^(1 / gamma) at its luminance — and a tile whose rms is at most the threshold is finished at the samples it has; its
	// `error` is that rms.  The threshold is a fraction of the display's full scale: 1 / 255 is one 8-bit level.  adaptive_display_floor: luminances that
	// display below it take the slope at it.  adaptive_display_auto_exposure: every check first takes the exposure its own histogram of the whole frame asks
	// for (auto_exposure_percentile, auto_exposure_target) in place of adaptive_display_exposure; one device.  render_tiled throws with adaptive_threshold,
	// with an adaptive_measure other than "channel_max" and with denoise_dual.
	double adaptive_display_threshold = 0.0;
	double adaptive_display_exposure = 1.0;
	double adaptive_display_gamma = 2.2;
	double adaptive_display_floor = 1.0 / 255.0;
	bool adaptive_display_auto_exposure = false;
	// Denoising (an extension; false = off): await() returns the assembled frame filtered by rmd_denoise (raymond_hip.h) with these parameters; the
	// passes then render with second moments and TileFinished tiles carry them in `data_sq`.  render_tiled throws raymond::Error for values
	// rmd_denoise refuses (radius <= 12, patch <= 4, k finite and > 0, alpha finite and >= 0).
	bool denoise = false;
	uint32_t denoise_radius = 10, denoise_patch = 3;
	double denoise_k = 0.45, denoise_alpha = 1.0;
	// Feature-guided denoising (needs denoise; false = off): await() also uploads the scene to its GPU, renders the finished tiles' first-hit features
	// there (rmd_render_features: one call per distinct sample count, each tile at its own count, this seed and DOF flag) and filters with
	// rmd_denoise_guided, k_f = denoise_feature_k, tau = denoise_feature_tau (both finite and > 0, or render_tiled throws).
	bool denoise_features = false;
	double denoise_feature_k = 1.0, denoise_feature_tau = 1e-2; // (the best of the sweep in DESIGN.md section 12)
	// The feature-slope term of the guided non-local-means filters (0 = off: no frame, message or launch changes): the pixels of a feature's local slope
	// that are not an edge (raymond_hip.h: rmd_denoise_guided_slope; 3 is the value to start from).  When set, whichever of denoise_features,
	// denoise_dual_features (await() and the adaptive check's region call) and denoise_dual_select's guided candidate is on makes its _slope call with it.
	// render_tiled throws if it is not finite or negative, if it is > 0 with none of the three on, or with denoise_atrous / denoise_dual_atrous.
	double denoise_feature_slope = 0.0;
	// The same term in the guided a-trous filters (0 = off: no frame, message or launch changes; raymond_hip.h: rmd_denoise_atrous_slope; 3 is the value to
	// start from).  When set, every call of a guided a-trous filter is its _slope call with it: await() with denoise_atrous + denoise_features or
	// denoise_dual_atrous + denoise_dual_features, the adaptive check (its region form with denoise_dual_atrous_region) and a filtered FramePreview when it is
	// guided.  render_tiled throws if it is not finite or negative, or if it is > 0 with neither of the two pairs on.
	double denoise_atrous_slope = 0.0;
	// The fast filter for previews (needs denoise, not with denoise_dual; false = off): await() returns rmd_denoise_atrous's frame at
	// denoise_atrous_levels (0..8) and k = denoise_atrous_k (finite and > 0) with denoise_alpha, guided by the first-hit features when
	// denoise_features is on (denoise_feature_k, denoise_feature_tau).  denoise_radius, denoise_patch and denoise_k are then not used.  render_tiled
	// throws for levels or k out of range whether or not the setting is on.
	bool denoise_atrous = false;
	uint32_t denoise_atrous_levels = 5;
	double denoise_atrous_k = 3.0;
	// Dual-buffer denoising (needs denoise and samples_per_iteration > 0, one GPU, not with denoise_features; false = off): pass j of a tile, counted
	// from 0, adds its samples to half A when j is even and to half B when j is odd; TileFinished tiles carry both halves and await() returns
	// rmd_denoise_dual's frame (raymond_hip.h).
	bool denoise_dual = false;
	// Feature weights in the dual-buffer filter (needs denoise_dual; false = off): the filter is rmd_denoise_dual_guided with the finished tiles' first-hit
	// features at count_a + count_b samples per tile, k_f = denoise_feature_k and tau = denoise_feature_tau; the adaptive check is its region form.
	bool denoise_dual_features = false;
	// Per-pixel choice among dual-buffer filters (needs denoise_dual; false = off): await() renders the finished tiles' features as denoise_dual_features
	// does and returns rmd_denoise_dual_select's frame at two candidates — (k = denoise_k, unguided) and (k = 1.0, guided, denoise_feature_k,
	// denoise_feature_tau), both at denoise_alpha — with both windows 2.  The adaptive check is untouched.
	bool denoise_dual_select = false;
	// The fast filter in the dual-buffer loop (needs denoise_dual, not with denoise_dual_select; false = off): await() returns rmd_denoise_atrous_dual's
	// frame at denoise_atrous_levels, denoise_atrous_k and denoise_alpha, guided when denoise_dual_features is on, and the adaptive check is that call on
	// the whole frame.
	bool denoise_dual_atrous = false;
	// The region form in that check (needs denoise_dual_atrous; false = off): the check calls rmd_denoise_atrous_dual_region over the live tiles, which gives
	// their pixels the whole-frame call's bytes at a cost that follows their dilated area.  No message and no output changes; await() is untouched.
	bool denoise_dual_atrous_region = false;
	// Adaptive sampling by the filtered frame's error (needs denoise_dual, excludes adaptive_threshold > 0; 0 = off): after every even number of
	// passes that leaves live tiles with at least adaptive_min_samples samples, rmd_denoise_dual runs over the whole frame and a live tile whose
	// rmd_tile_error_dual — an absolute RMS in linear radiance that reads low — is at most the threshold is finished at the samples it has.
	double adaptive_denoised_threshold = 0.0;
	size_t adaptive_min_samples = 32;
	// Adaptive sampling by the DISPLAYED error of the filtered frame (needs denoise_dual and samples_per_iteration > 0, excludes
	// adaptive_denoised_threshold > 0 and adaptive_threshold > 0; 0 = off): the same checks at the same passes, but after the filter call one
	// rmd_tile_weighted_error_dual call over the live tiles — the filter's error image weighted, by the filtered frame's luminance, under rmd_display_weights'
	// table at adaptive_display_exposure, adaptive_display_gamma and adaptive_display_floor (adaptive_display_auto_exposure: at the exposure every check's own
	// histogram of the whole frame's raw sums asks for) — and a tile whose rms is at most the threshold is finished.  A fraction of the display's full scale.
	double adaptive_denoised_display_threshold = 0.0;
	// Frame previews during a progressive render (needs samples_per_iteration > 0; 0 = off): after every preview_every-th pass that leaves the render
	// unfinished — the passes after which TileProgressed is sent — one Message::FramePreview follows that pass's TileProgressed messages: the whole frame
	// as W*H*3 bytes, every tile resolved and tone-mapped on the GPU at its own sample count (rmd_resolve_tonemap_tiles) with preview_exposure and
	// preview_gamma (both finite and > 0).  In this mirror a tile may move from GPU to GPU between passes, so no GPU holds a frame's share: previews
	// need worker_count == 1, and render_tiled throws otherwise.
	size_t preview_every = 0;
	double preview_exposure = 1.0, preview_gamma = 2.2;
	// The preview is the fast filter's frame instead of the raw means (needs preview_every; false = off), at denoise_atrous_levels, denoise_atrous_k and
	// denoise_alpha: rmd_denoise_atrous on the sums and sums of squares — the passes then render with second moments, as they do for denoise —, in the
	// dual-buffer loop rmd_denoise_atrous_dual, guided by the feature buffers when the loop already keeps them.  Its means are resolved at count 1.
	bool preview_denoise = false;
	// false: no TileProgressed message is made and nothing is downloaded for one; an adaptive render's TileFinished messages stay.
	bool progress_tiles = true;
	// Automatic exposure for the previews (needs preview_every; false = off): every preview first takes the luminance histogram of exactly the buffers, rects
	// and counts its rmd_resolve_tonemap_tiles call is about to use (rmd_luminance_histogram_tiles), and the exposure that puts the
	// auto_exposure_percentile (finite, in (0, 1]) of luminance at auto_exposure_target (finite, in (0, 1)) before gamma — rmd_exposure_from_histogram —
	// replaces preview_exposure in that call; Preview::exposure carries it.  0.99 and 0.8 are values to start from.
	bool preview_auto_exposure = false;
	double auto_exposure_percentile = 0.99, auto_exposure_target = 0.8;
	// Firefly rejection in front of everything that reads the moments (false = off: no buffer, launch or copy is added).  await() despikes the assembled
	// sums and sums of squares on its GPU (raymond_hip.h: rmd_despike at despike_radius 1..3, despike_rank <= (2 * radius + 1)^2 - 2, despike_k finite and
	// >= 0, despike_ratio finite and >= 1, despike_floor finite and >= 0) before the plain divide, denoise, denoise_features or denoise_atrous; the passes then
	// render with second moments, as for denoise.  The adaptive_threshold check despikes all tiles at their current counts into two spare buffers and runs
	// rmd_tile_error on those (worker_count == 1 only); the sums the passes add to, every message's data and the previews stay the raw sums.  render_tiled
	// throws for values out of range whether or not the setting is on, with denoise_dual (whose halves despike_dual despikes) and with adaptive_threshold on
	// several workers.  2, 2, 6, 2 and 0 are values to start from.
	bool despike = false;
	uint32_t despike_radius = 2, despike_rank = 2;
	double despike_k = 6.0, despike_ratio = 2.0, despike_floor = 0.0;
	// Firefly rejection for the two halves of the dual-buffer paths (false = off: no buffer, launch or copy is added; needs denoise_dual), at the five
	// despike_* values above (raymond_hip.h: rmd_despike_dual).  await() despikes the assembled halves on its GPU before whichever dual filter the settings
	// choose.  In the dual loop every call of the dual filter — the adaptive check and the filtered preview — reads despiked copies: four spare buffers,
	// filled once per pass by one rmd_despike_dual call over the whole frame, finished tiles at the counts they finished with and live tiles at n_A / n_B.
	// The sums the passes add to, every message's data, raw previews and the auto-exposure histogram stay the raw sums.
	bool despike_dual = false;
};
// What render_tiled refuses in the preview settings (it throws this text as a raymond::Error); empty: nothing.  One policy with raymond_amd/scene.py's
// Settings.check_preview.
std::string check_preview(const Settings &settings);

// core/src/tile.rs:13 `data: Vec<Vector3>` — the running sums of a tile, width * height of them, row-major.  Here a VIEW: the tiles of one
// message batch (a progressive pass's TileProgressed snapshots, or the TileFinished tiles) share the one page-locked block their pixels were
// downloaded into (rmd_framebuffer_download_tiles: the block is in Tile.data layout already), kept alive by its last tile — where the
// reference clones 24 KB per tile and message (src/trace.rs:212,218).  A tile that was not produced by a download owns its block.
class TileData {
  public:
	TileData() = default;
	explicit TileData(size_t n) : block_(new Vector3[n](), std::default_delete<Vector3[]>()), p_(static_cast<Vector3 *>(block_.get())), n_(n) {}
	TileData(std::shared_ptr<void> block, Vector3 *first, size_t n) : block_(std::move(block)), p_(first), n_(n) {}
	size_t size() const { return n_; }
	bool empty() const { return n_ == 0; }
	const Vector3 &operator[](size_t i) const { return p_[i]; }
	Vector3 &operator[](size_t i) { return p_[i]; }
	const Vector3 *data() const { return p_; }
	Vector3 *data() { return p_; }
	const Vector3 *begin() const { return p_; }
	const Vector3 *end() const { return p_ + n_; }
	void push_back(const Vector3 &v) { // (tests build small tiles by hand)
		TileData grown(n_ + 1);
		for (size_t i = 0; i < n_; i++) grown[i] = p_[i];
		grown[n_] = v;
		*this = std::move(grown);
	}

  private:
	std::shared_ptr<void> block_;
	Vector3 *p_ = nullptr;
	size_t n_ = 0;
};
struct Tile { // core/src/tile.rs:7-14
	size_t sample_count = 0, width = 0, height = 0, left = 0, top = 0;
	TileData data; // running sums, width*height.  EMPTY while the tile waits in the queue with its sums resident on a GPU (`resident`)
	int resident = -1; // the worker (GPU) whose device framebuffer holds the tile's sums; -1: `data` does (an extension: the reference's tiles live in RAM)
	TileData data_sq;  // adaptive renders with several GPUs: the running sums of squares (rmd_render_tiles_moments), travelling through RAM with `data`
	                   // while the tile waits in the queue; denoised renders: also every TileFinished tile's; empty otherwise
	// dual-buffer renders (settings.denoise_dual): a TileFinished tile's two sample halves — sums, sums of squares and samples per pixel —; `data` and
	// `data_sq` are then the halves' sums added and sample_count = count_a + count_b.  Empty / 0 otherwise
	TileData data_a, data_sq_a, data_b, data_sq_b;
	size_t count_a = 0, count_b = 0;
	// dual-buffer adaptive renders: the tile's rmd_tile_error_dual when it was last checked; adaptive renders by a luma measure (settings.adaptive_measure):
	// its rmd_tile_luma_error tile_rms or pixel_rms, whichever decides; adaptive renders by the displayed error (settings.adaptive_display_threshold): its
	// rmd_tile_weighted_error rms; -1: never
	double error = -1.0;
};
// An extension (settings.preview_every): the frame after pass `pass_index` (counted from 1), row-major RGB bytes; sample_count: the samples per pixel
// of a tile that is still live (tiles that finished early are in the frame at the count they finished with)
struct Preview {
	std::vector<uint8_t> rgb8;
	size_t width = 0, height = 0, pass_index = 0, sample_count = 0;
	std::optional<double> exposure; // settings.preview_auto_exposure: the exposure the frame's histogram asked for and was tone-mapped with; unset when it is off
};
struct Message { // src/trace.rs:62-66
	enum Kind { TileFinished, TileProgressed, FramePreview } kind; // FramePreview: `preview` is set and `tile` is empty
	Tile tile;
	std::shared_ptr<const Preview> preview = nullptr;
};

// src/trace.rs:70-135
class TaskHandle {
  public:
	using TileCallback = std::function<void(const Tile &)>;
	Settings settings;
	void set_callback(TileCallback cb) { callback_ = std::move(cb); }
	using PreviewCallback = std::function<void(const Preview &)>;
	void set_preview_callback(PreviewCallback cb) { preview_callback_ = std::move(cb); }
	// Blocks until every worker is done, then assembles W*H radiance values (tile sums / sample_count), row-major (:82-113).  settings.denoise: the
	// collected tiles go through denoise_tiles (settings.denoise_dual: denoise_dual_tiles) on GPU 0 instead (none collected: the zero frame, as without it)
	std::vector<Vector3> await();
	std::optional<Message> poll();        // :115-117
	void async_await();                   // :119-134: drains leading TileProgressed messages into the callback (and FramePreview ones into the preview callback)
	bool finished() const;                // extension: alive_thread_count == 0 (what await() polls for, :89)
	double setup_seconds() const;         // extension (measurement): the longest a worker took to get ready — context, scene upload, framebuffer
	~TaskHandle();
	TaskHandle(TaskHandle &&) = default;
	struct Shared; // queue + channel shared with the workers (implementation detail)

  private:
	friend TaskHandle render_tiled(const Scene &, const Settings &);
	TaskHandle() = default;
	std::shared_ptr<const Scene> scene_; // settings.denoise_features / denoise_dual_features: the scene whose features await() renders
	std::shared_ptr<Shared> shared_;
	std::vector<std::thread> workers_;
	TileCallback callback_;
	PreviewCallback preview_callback_;
};

// src/trace.rs:137-230
TaskHandle render_tiled(const Scene &scene, const Settings &settings);

// Extension (settings.denoise): the W*H denoised means, row-major — the tiles' sums (`data`), sums of squares (`data_sq`) and sample counts
// assembled into one frame and filtered by rmd_denoise on GPU `device` with the settings' parameters.  A pixel that no tile covers has n = 0 (0 / 0).
// settings.denoise_features: `scene` (required then) is uploaded to that GPU, the tiles' first-hit features are rendered and the filter is
// rmd_denoise_guided.  feature_means (optional): receives the W*H*7 feature means (sums / the tile's count; 0 / 0 where no tile lies).
std::vector<Vector3> denoise_tiles(const std::vector<Tile> &tiles, const Settings &settings, int device = 0, const Scene *scene = nullptr,
                                   std::vector<double> *feature_means = nullptr);
// Extension (settings.denoise_dual): the W*H means of rmd_denoise_dual on GPU `device` over the tiles' two halves (data_a .. count_b) with the
// settings' parameters.  tile_errors (optional): receives rmd_tile_error_dual of every tile, in the tiles' order.  settings.denoise_dual_features: `scene`
// (required then) is uploaded to that GPU, the tiles' first-hit features are rendered at count_a + count_b samples and the filter is rmd_denoise_dual_guided.
// settings.denoise_dual_select: the scene and the features likewise, and the frame is rmd_denoise_dual_select's at the setting's two candidates.
std::vector<Vector3> denoise_dual_tiles(const std::vector<Tile> &tiles, const Settings &settings, int device = 0, std::vector<double> *tile_errors = nullptr,
                                        const Scene *scene = nullptr);
// The W*H*7 first-hit feature sums (and, when asked for, sums of squares) of a frame whose rect i holds counts[i] samples, rendered on GPU `device`
// with the settings' camera, seed and DOF flag: the AOVs (normal xyz, albedo rgb, depth) of raymond_hip.h's rmd_render_features.
std::vector<double> render_features(const Scene &scene, const Settings &settings, const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts,
                                    int device = 0, std::vector<double> *sums_sq = nullptr);
// The W*H*RMD_ID_WORDS first-hit ID words (raymond_hip.h's rmd_render_ids: per pixel key_0 count_0 .. key_3 count_3 other samples) of a frame whose rect i
// holds counts[i] samples, rendered on GPU `device` with the settings' camera, seed and DOF flag: one call per distinct count.
std::vector<uint32_t> render_ids(const Scene &scene, const Settings &settings, const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts, int device = 0);
// rmd_ids_matte on GPU `device` over host words: per pixel the share of its samples whose first hit is one of `objects` (indices; RMD_ID_MISS: the
// background).  other_pixels (optional): the pixels whose table overflowed, where the matte is a lower bound.
std::vector<double> ids_matte(const std::vector<uint32_t> &words, size_t width, size_t height, const std::vector<uint32_t> &objects, int device = 0,
                              uint64_t *other_pixels = nullptr);
// ... and on the host, from the header the kernel is built from (raymond_amd/csrc/ids_rule.hpp): no GPU.  What raymond_cli ids-matte runs, and what holds
// the header to the numpy restatement
std::vector<double> ids_matte_host(const std::vector<uint32_t> &words, size_t width, size_t height, const std::vector<uint32_t> &objects, uint64_t *other_pixels = nullptr);

// The W*H*RMD_AO_WORDS ambient-occlusion words (raymond_hip.h's rmd_render_ao: per pixel occluded open none samples, the diffuse bounce ray off the first
// hit tested against max_distance) of a frame whose rect i holds counts[i] samples, rendered on GPU `device` with the settings' camera, seed and DOF
// flag: one call per distinct count.
std::vector<uint32_t> render_ao(const Scene &scene, const Settings &settings, const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts, double max_distance,
                                int device = 0);
// rmd_ao_resolve on GPU `device` over host words: per pixel open / (open + occluded), empty_value where no sample has a first hit.  empty_pixels
// (optional): the number of such pixels.
std::vector<double> ao_resolve(const std::vector<uint32_t> &words, size_t width, size_t height, double empty_value = 1.0, int device = 0, uint64_t *empty_pixels = nullptr);
// ... and on the host, from the header the kernel is built from (raymond_amd/csrc/ao_rule.hpp): no GPU.  What raymond_cli ao-resolve runs, and what holds
// the header to the numpy restatement
std::vector<double> ao_resolve_host(const std::vector<uint32_t> &words, size_t width, size_t height, double empty_value = 1.0, uint64_t *empty_pixels = nullptr);

// Closest-hit queries for the caller's own rays (raymond_hip.h's rmd_intersect_rays): rays holds 6 doubles a ray — origin xyz, direction xyz, the direction
// used as given —, the result one rmd_ray_hit a ray (a miss: object -1, t 0, a zero normal, triangle 0).  The scene is uploaded to GPU `device` for the call.
std::vector<rmd_ray_hit> intersect_rays(const Scene &scene, const std::vector<double> &rays, int device = 0);
// rmd_camera_rays on GPU `device`: the pinhole primary rays of the settings' camera for the pixels xy (x, y pairs) at the jitter uniforms uv (pairs, or
// null: 0.5, 0.5 — the pixel centres), 6 doubles a ray
std::vector<double> camera_rays(const Settings &settings, const std::vector<uint32_t> &xy, const std::vector<double> *uv = nullptr, int device = 0);
// What pixel (x, y) of the settings' camera sees through its centre: the ray is made and intersected on the device
rmd_ray_hit pick(const Scene &scene, const Settings &settings, uint32_t x, uint32_t y, int device = 0);

// rmd_resolve_tonemap_tiles on `ctx`: the rects of the width x height device framebuffer `accum_dev`, rect i at counts[i] samples per pixel, tone-mapped
// into packed bytes — rect after rect, each row-major, 3 bytes per pixel.  accum2_dev (or null): a dual-buffer render's other half, added first.
std::vector<uint8_t> resolve_tonemap_tiles(rmd_context *ctx, const double *accum_dev, const double *accum2_dev, size_t width, size_t height,
                                           const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts, double exposure = 1.0, double gamma = 2.2);
// ... and those packed bytes written into a width x height x 3 frame at their rects (later rects overwrite earlier ones where they overlap)
void scatter_tiles(const std::vector<rmd_tile_rect> &rects, const std::vector<uint8_t> &packed, size_t width, size_t height, std::vector<uint8_t> &frame);

// Tile generation of render_tiled (:142-173): column-major, edge tiles clamped
std::vector<rmd_tile_rect> generate_tiles(size_t width, size_t height, std::pair<size_t, size_t> tile_size);
// A tile's place in the frame, as the C-ABI takes it
rmd_tile_rect rect_of(const Tile &tile);
// Frame assembly (:93-99): `data` — one of the tile's TileData, width * height of them — written into the row-major frame `width` pixels wide at the
// tile's rect, every value divided by `divisor` (await(): the tile's sample_count)
void place_tile(const Tile &tile, const TileData &data, size_t width, std::vector<Vector3> &frame, double divisor = 1.0);
// width * height * channels sums divided by the count of the rect their pixel lies in (rect i holds counts[i] samples; 0 / 0 where no rect lies)
void divide_by_counts(std::vector<double> &sums, size_t width, size_t height, size_t channels, const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts);

// The luminance histogram of a host image of radiance means: rmd_luminance_histogram_tiles's counters (the same luminance and binning, read from the
// header the kernel is built from) with every pixel at a count of 1 — what the final frame's automatic exposure is made from
// (rmd_exposure_from_histogram; raymond_cli --auto-exposure 1)
rmd_luma_histogram luminance_histogram(const std::vector<Vector3> &image);

// rmd_despike on the host, from the header the kernel is built from (raymond_amd/csrc/despike_rule.hpp): width * height sums and sums of squares in, the
// despiked ones out (out_sums / out_sums_sq are resized), the spikes per rect returned.  No argument is checked beyond the sizes; rects are inside the
// frame and disjoint.  What raymond_cli despike runs, and what holds the header to the numpy restatement without a GPU
std::vector<uint32_t> despike_host(const std::vector<Vector3> &sums, const std::vector<Vector3> &sums_sq, size_t width, size_t height, const std::vector<rmd_tile_rect> &rects,
                                   const std::vector<uint32_t> &counts, uint32_t radius, uint32_t rank, double k, double ratio, double floor,
                                   std::vector<Vector3> &out_sums, std::vector<Vector3> &out_sums_sq);
// rmd_despike_dual on the host, from the headers the kernel is built from (raymond_amd/csrc/despike_dual_rule.hpp over despike_rule.hpp): the two halves'
// sums and sums of squares in, the four despiked buffers out (resized), the spikes per rect returned.  Checked: the sizes, the radius and that no rect's two
// counts add past 2^32 - 1; rects are inside the frame and disjoint.  What raymond_cli despike-dual runs
std::vector<uint32_t> despike_dual_host(const std::vector<Vector3> &sums_a, const std::vector<Vector3> &sums_sq_a, const std::vector<Vector3> &sums_b,
                                        const std::vector<Vector3> &sums_sq_b, size_t width, size_t height, const std::vector<rmd_tile_rect> &rects,
                                        const std::vector<uint32_t> &counts_a, const std::vector<uint32_t> &counts_b, uint32_t radius, uint32_t rank, double k, double ratio,
                                        double floor, std::vector<Vector3> &out_a, std::vector<Vector3> &out_sq_a, std::vector<Vector3> &out_b, std::vector<Vector3> &out_sq_b);
// rmd_tile_luma_error on the host, from the header the kernel is built from (raymond_amd/csrc/tile_luma_rule.hpp: 256 emulated lanes and the kernel's
// combine): rect i of the width * height sums and sums of squares at counts[i].  No argument is checked beyond the sizes; rects are inside the frame.  What
// raymond_cli tile-luma-error runs, and what holds the header to the numpy restatement without a GPU
std::vector<rmd_tile_luma> tile_luma_error_host(const std::vector<Vector3> &sums, const std::vector<Vector3> &sums_sq, size_t width, size_t height,
                                                const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts, double floor);
// rmd_tile_weighted_error on the host, from the header the kernel is built from (raymond_amd/csrc/tile_weighted_rule.hpp: 256 emulated lanes and the kernel's
// combine): rect i of the width * height sums and sums of squares at counts[i], under `weights` (RMD_LUMA_WEIGHTS entries).  No argument is checked beyond
// the sizes; rects are inside the frame.  What raymond_cli tile-weighted-error runs, and what holds the header to the numpy restatement without a GPU
std::vector<rmd_tile_weighted> tile_weighted_error_host(const std::vector<Vector3> &sums, const std::vector<Vector3> &sums_sq, size_t width, size_t height,
                                                        const std::vector<rmd_tile_rect> &rects, const std::vector<uint32_t> &counts, const std::vector<double> &weights);
// rmd_tile_weighted_error_dual on the host, from the header the kernel is built from (raymond_amd/csrc/tile_weighted_dual_rule.hpp): rect i of the
// width * height filtered means `out` and error image `err`, under `weights` (RMD_LUMA_WEIGHTS entries).  No argument is checked beyond the sizes; rects
// are inside the frame.  What raymond_cli tile-weighted-error-dual runs, and what holds the header to the numpy restatement without a GPU
std::vector<rmd_tile_weighted> tile_weighted_error_dual_host(const std::vector<Vector3> &out, const std::vector<double> &err, size_t width, size_t height,
                                                             const std::vector<rmd_tile_rect> &rects, const std::vector<double> &weights);
// rmd_display_weights: the RMD_LUMA_WEIGHTS weights of the displayed error at an exposure, a gamma and a display floor; throws for arguments it refuses
std::vector<double> display_weights(double exposure, double gamma, double display_floor);
// await() with settings.despike alone: the finished tiles' sums and sums of squares assembled, despiked on `device` (rmd_despike) and divided by each
// tile's count
std::vector<Vector3> despike_tiles(const std::vector<Tile> &tiles, const Settings &settings, int device);

// cli_old/src/main.rs:155-181 on the host: c = (1 - exp(-p * exposure))^(1/gamma); u8 = trunc(c * 255)
std::vector<uint8_t> tone_map(const std::vector<Vector3> &image, double exposure = 1.0, double gamma = 2.2);
void write_ppm(const std::string &path, const std::vector<uint8_t> &rgb8, size_t width, size_t height);

// core/src/project.rs:13-57 — the scene file: serde-JSON, enums externally tagged ({"Plane":{..}} | {"Sphere":{..}} |
// {"Mesh":"file.ply"}; {"Diffuse":[V,r]} | {"Metal":[V,r]} | {"Emission":[V,V,f,f]}), Vector3 as {"x","y","z"} or [x,y,z].
struct ProjectObject {
	enum Kind { PlaneGeometry, SphereGeometry, MeshGeometry } kind = PlaneGeometry;
	Plane plane{};
	Sphere sphere{};
	std::string mesh_path; // Geometry::Mesh(PathBuf)
	Material material{};
};
struct Project {
	std::vector<ProjectObject> objects;
	std::string base_dir; // directory of the project file: relative mesh paths are resolved against it (as raymond_amd/project.py does)
	static Project load(const std::string &path);                                       // project.rs:33-36
	static Project loads(const std::string &json_text, const std::string &base_dir = ""); // serde_json::from_str
	std::string dumps() const;                                                           // serde_json::to_string
	Scene build_scene() const; // project.rs:38-57: meshes through Mesh::load_ply + AccGrid::build_from_mesh
};
// server/src/protocol.rs:9-14: {"type":"TileProgressed"|"TileFinished","data":{sample_count,width,height,left,top,data:[V..]}}
// (a FramePreview has no wire form there: raymond::Error)
std::string message_to_json(const Message &message);

// Benchmark inputs, identical to raymond_amd/scenes.py
Scene reflective_spheres();
Mesh lumpy_sphere_mesh(int n = 91, Vector3 extent = {2.3, 1.7, 1.0}, Vector3 centre = {0.0, 0.15, 0.0});
Scene gold_dragon_standin(int n = 91);

} // namespace raymond
