// C-ABI implementation (include/raymond_hip.h): contexts, the error plumbing, and everything that plans and launches a render.  Scene upload is in
// api_scene.cpp; framebuffers, tile transfers, the resolve/tone-map epilogue and the histogram in api_frame.cpp; the denoise entry points and the
// per-tile measures in api_denoise.cpp.  Host code only; kernels are in kernels.hip.
#define RMD_WITH_HIP 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <new>

#include "ids_rule.hpp"
#include "internal.hpp"
#include "launch.hpp"

using rmd::bind;

namespace {
thread_local std::string tl_last_error;

rmd_status context_create(int32_t device, hipStream_t stream, bool own_stream, rmd_context **out) {
	if (!out) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "rmd_context_create: null out pointer");
	*out = nullptr;
	int count = 0;
	hipError_t e = hipGetDeviceCount(&count);
	if (e != hipSuccess || count <= 0)
		return rmd::fail(nullptr, RMD_ERR_NO_DEVICE, std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
	if (device < 0 || device >= count) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "rmd_context_create: device ordinal out of range");
	RMD_HIP(nullptr, hipSetDevice(device));
	hipDeviceProp_t prop;
	RMD_HIP(nullptr, hipGetDeviceProperties(&prop, device));
	if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
		return rmd::fail(nullptr, RMD_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only");
	std::unique_ptr<rmd_context> ctx(new (std::nothrow) rmd_context()); // (an early return below destroys what exists by then: ~rmd_context)
	if (!ctx) return rmd::fail(nullptr, RMD_ERR_OUT_OF_MEMORY, "rmd_context_create: allocation failed");
	ctx->device = device;
	ctx->n_cus = (uint32_t)prop.multiProcessorCount;
	ctx->wave_slots = (uint32_t)prop.multiProcessorCount * 16u; // both render kernels fit 4 waves per SIMD (<= 128 VGPRs)
	ctx->owns_stream = own_stream, ctx->stream = stream;
	if (own_stream) {
		hipError_t se = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
		if (se != hipSuccess) {
			ctx->stream = nullptr; // nothing for ~rmd_context to wait for or destroy
			return rmd::fail(nullptr, RMD_ERR_HIP, std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(se));
		}
	}
	// environment hooks are read here, once; rmd_context_set_tunable changes them afterwards
	{
		auto env_int = [](const char *name) -> int64_t {
			const char *v = std::getenv(name);
			return v ? (int64_t)std::atoll(v) : 0;
		};
		ctx->tunable[RMD_TUNE_SAMPLE_SPLIT] = env_int("RMD_SAMPLE_SPLIT");
		ctx->tunable[RMD_TUNE_WALK_BATCH] = env_int("RMD_WALK_BATCH");
		ctx->tunable[RMD_TUNE_MASK_BUDGET] = env_int("RMD_MASK_BUDGET");
		ctx->tunable[RMD_TUNE_SCRATCH_CAP_MB] = env_int("RMD_SCRATCH_CAP_MB");
		ctx->tunable[RMD_TUNE_WALK_CUT] = env_int("RMD_WALK_CUT");
		ctx->tunable[RMD_TUNE_SPLIT_MIN_SAMPLES] = env_int("RMD_SPLIT_MIN_SAMPLES");
		ctx->tunable[RMD_TUNE_CHAIN_ITEMS] = env_int("RMD_CHAIN_ITEMS");
		ctx->tunable[RMD_TUNE_AXIS_PAIRS] = env_int("RMD_AXIS_PAIRS");
		ctx->tunable[RMD_TUNE_PATH_QUEUES] = env_int("RMD_PATH_QUEUES");
		const char *form = std::getenv("RMD_LAUNCH_FORM");
		ctx->tunable[RMD_TUNE_LAUNCH_FORM] = !form ? 0 : (std::strcmp(form, "per-item") == 0 || std::strcmp(form, "1") == 0) ? 1 : (std::strcmp(form, "persistent") == 0 || std::strcmp(form, "2") == 0) ? 2 : 0;
#if RMD_DIAG
		ctx->debug_flags = (uint32_t)env_int("RMD_DEBUG"); // DIAG builds only: 1 | 2 are timing ablations that change results, 8 | 16 count events, 256 fails the path queues' allocation, 1024 makes the work list's tail 4 wave tiles
#endif
#if RMD_WORK_LIST_SWEEP
		// sweep builds only (tools/work_list_sweep.py): RMD_WORK_LIST = "<tail tiles per wave slot, in halves>,<parts of a tail tile>"; 0 halves = no whole items
		if (const char *v = std::getenv("RMD_WORK_LIST")) {
			unsigned a = 0, b = 0;
			if (std::sscanf(v, "%u,%u", &a, &b) == 2 && b >= 1u) ctx->tail_x2 = a, ctx->tail_parts = b;
		}
#endif
	}
	if (hipEventCreate(&ctx->ev_start) != hipSuccess || hipEventCreate(&ctx->ev_stop) != hipSuccess)
		return rmd::fail(nullptr, RMD_ERR_HIP, "hipEventCreate failed");
	// the fault words: pinned host memory the device writes through (coherent: visible to the host once the launch has completed)
	{
		void *h = nullptr, *d = nullptr;
		hipError_t fe = hipHostMalloc(&h, rmd::kFaultWords * sizeof(uint32_t), hipHostMallocMapped);
		if (fe == hipSuccess) {
			ctx->h_fault = (uint32_t *)h;
			std::memset(h, 0, rmd::kFaultWords * sizeof(uint32_t));
			fe = hipHostGetDevicePointer(&d, h, 0);
		}
		if (fe != hipSuccess) return rmd::fail(nullptr, RMD_ERR_HIP, std::string("fault words (hipHostMalloc): ") + hipGetErrorString(fe));
		ctx->d_fault = (uint32_t *)d;
	}
	*out = ctx.release();
	return RMD_OK;
}

// Splits host tiles (core::tile::Tile rectangles) into 8x8 wave tiles; cached per context while the
// rect list stays the same (a progressive render re-submits the same tiles every pass).
rmd_status prepare_wave_tiles(rmd_context *ctx, const rmd_camera *cam, const rmd_tile_rect *tiles, uint32_t n_tiles) {
	const uint32_t W = cam->backbuffer_width, H = cam->backbuffer_height;
	if (ctx->wave_tiles.bytes() && ctx->cached_W == W && ctx->cached_H == H && ctx->cached_rects.size() == n_tiles &&
	    (n_tiles == 0 || std::memcmp(ctx->cached_rects.data(), tiles, sizeof(rmd_tile_rect) * n_tiles) == 0))
		return RMD_OK;
	std::vector<rmd::WaveTile> wt;
	for (uint32_t i = 0; i < n_tiles; i++) {
		const rmd_tile_rect &r = tiles[i];
		if (r.width == 0 || r.height == 0) continue; // (a rect without pixels may lie outside the frame here; rmd::rects_inside would refuse it)
		if ((uint64_t)r.left + r.width > W || (uint64_t)r.top + r.height > H)
			return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_render_tiles: tile rectangle outside the backbuffer");
		for (uint32_t y = r.top; y < r.top + r.height; y += 8)
			for (uint32_t x = r.left; x < r.left + r.width; x += 8) {
				rmd::WaveTile t;
				t.x0 = (uint16_t)x, t.y0 = (uint16_t)y;
				t.w = (uint8_t)((r.left + r.width - x) < 8u ? (r.left + r.width - x) : 8u);
				t.h = (uint8_t)((r.top + r.height - y) < 8u ? (r.top + r.height - y) : 8u);
				t._pad = 0;
				wt.push_back(t);
			}
	}
	RMD_HIP(ctx, ctx->wave_tiles.grow(wt.size() * sizeof(rmd::WaveTile)));
	if (!wt.empty()) {
		RMD_HIP(ctx, hipMemcpyAsync(ctx->wave_tiles.as<rmd::WaveTile>(), wt.data(), wt.size() * sizeof(rmd::WaveTile), hipMemcpyHostToDevice, ctx->stream));
		RMD_HIP(ctx, hipStreamSynchronize(ctx->stream)); // wt is a stack-owned staging vector
	}
	ctx->n_wave_tiles = (uint32_t)wt.size();
	ctx->cached_rects.assign(tiles, tiles + n_tiles);
	ctx->cached_W = W, ctx->cached_H = H;
	return RMD_OK;
}

rmd_status check_render_args(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *cam, const rmd_settings *st) {
	if (!scene || !cam || !st) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "render: null scene/camera/settings");
	if (scene->ctx != ctx) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "render: scene belongs to another context");
	if (cam->backbuffer_width == 0 || cam->backbuffer_height == 0 || cam->backbuffer_width > 65535u || cam->backbuffer_height > 65535u)
		return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "render: backbuffer size must be 1..65535 per axis");
	if (st->bounce_limit > RMD_MAX_BOUNCE_LIMIT) return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "render: bounce_limit above RMD_MAX_BOUNCE_LIMIT");
	if ((uint64_t)st->sample_begin + st->sample_count > 0xFFFFFFFFull) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "render: sample range overflows u32");
	if (st->flags & ~(RMD_RENDER_DOF | RMD_RENDER_TRACE_BLACK_PATHS | RMD_RENDER_END_BLACK_PATHS)) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "render: unknown bits in rmd_settings.flags");
	if ((st->flags & RMD_RENDER_TRACE_BLACK_PATHS) && (st->flags & RMD_RENDER_END_BLACK_PATHS))
		return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "render: RMD_RENDER_TRACE_BLACK_PATHS and RMD_RENDER_END_BLACK_PATHS exclude each other");
	if (rmd::render_lds_bytes(scene->n_objects, scene->mask_words_total, 1) + (scene->n_grids == 0u ? rmd::kSortPoolBytes : 0u) > rmd::kLdsBudgetBytes) // (one wave's area, head included)
		return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "render: object table + grid masks exceed the 160 KiB LDS of a CU");
	return RMD_OK;
}

} // namespace

namespace rmd {

rmd_status fail(rmd_context *ctx, rmd_status status, const std::string &text) {
	if (ctx) ctx->last_error = text;
	tl_last_error = text;
	return status;
}

rmd_status fail_noexcept(rmd_context *ctx, rmd_status status, const char *what, const char *text) noexcept {
	try {
		return fail(ctx, status, std::string(what) + ": " + text);
	} catch (...) { // not even the message: the status alone
		try {
			if (ctx) ctx->last_error.clear();
			tl_last_error.clear();
		} catch (...) {
		}
		return status;
	}
}

rmd_status bind(rmd_context *ctx) {
	if (!ctx) return fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "null context");
	RMD_HIP(ctx, hipSetDevice(ctx->device));
	return RMD_OK;
}

static_assert(RMD_MAX_BOUNCE_LIMIT_DEV == RMD_MAX_BOUNCE_LIMIT, "launch.hpp mirrors include/raymond_hip.h");

// Called after every wait for the context's stream.  The words are host memory: two loads when nothing happened.
rmd_status check_fault(rmd_context *ctx) {
	if (!ctx || !ctx->h_fault) return RMD_OK;
	volatile uint32_t *f = ctx->h_fault;
	const uint32_t code = f[0];
	if (code == 0u) return RMD_OK;
	const uint32_t item = f[1], reports = f[2];
	f[0] = 0u, f[1] = 0u, f[2] = 0u; // the next launch starts clean
	std::string what;
	if (code & kFaultTripLoop) what += " trip loop of render_wave;";
	if (code & kFaultSortedTripLoop) what += " trip loop of render_wave_sorted;";
	if (code & kFaultWorkLoop) what += " work loop of a persistent workgroup;";
	if (code & kFaultWalkRounds) what += " round loop of a grid walk;";
	if (code & kFaultQueuedTripLoop) what += " trip loop of render_wave_queued;";
	if (code & ~(kFaultTripLoop | kFaultSortedTripLoop | kFaultWorkLoop | kFaultWalkRounds | kFaultQueuedTripLoop)) what += " unknown code;";
	char num[96];
	std::snprintf(num, sizeof(num), " %u wave(s) reported, the last one at work item %u (code 0x%x)", reports, item, code);
	return fail(ctx, RMD_ERR_DEVICE_FAULT,
	            "device fault: a loop of the render kernel ran past its bound —" + what + num +
	                "; the launch was cut short and the framebuffer it wrote to is not valid");
}

// The launch's half of the conditions under which the generation trips get candidate sets of their own (primary_candidates.hpp): no thin lens
// and a finite camera; the scene's half — regular, no grid, not switched off — is rmd_scene::primary_cull.
bool primary_cull_allowed(const RenderParams &P) {
	CullCamera c;
	for (int a = 0; a < 3; a++) c.pos[a] = P.cam_pos[a];
	c.width = P.width, c.height = P.height, c.aspect = P.aspect, c.tan_half_fov = P.tan_half_fov;
	return P.use_dof == 0u && cull_camera_ok(c);
}

// Does the camera lie ON a plane of the scene?  A primary ray that faces such a plane hits it at t = 0 (plane.rs:11-24: t >= 0 counts), the hit
// point IS the camera position, and the view direction normalize(camera - hit) (src/trace.rs:257) is NaN: a non-finite weight from finite inputs,
// in a scene of regular parameters.  The reference's sample is then NaN unless the plane emits, so the two rules that end a path with L = 0 — a hit
// at the bounce limit, a diffuse bounce off a black surface — do not hold for such a launch (make_params).  "On": the numerator dot(o - cam, -n) of
// the plane test is zero, or so small (1e-9 of the sum of its terms' magnitudes: a distance no frame shows) that cam + t rd may round to cam.
bool camera_on_a_plane(const std::vector<double> &planes, const rmd_camera *cam) {
	for (size_t i = 0; i + 6 <= planes.size(); i += 6) {
		const double *o = &planes[i], *n = o + 3;
		double num = 0.0, scale = 0.0;
		for (int a = 0; a < 3; a++) num += (o[a] - cam->position[a]) * -n[a], scale += (std::fabs(o[a]) + std::fabs(cam->position[a])) * std::fabs(n[a]);
		if (!(std::fabs(num) > 1e-9 * scale)) return true; // (a NaN too)
	}
	return false;
}

// generate_primary_ray's loop-invariant terms (src/trace.rs:323-330), evaluated with the host libm
RenderParams make_params(const rmd_context *ctx, const rmd_scene *scene, const rmd_camera *cam, const rmd_settings *st) {
	const double PI = 3.14159265358979323846;
	RenderParams P;
	std::memset(&P, 0, sizeof(P));
	for (int a = 0; a < 3; a++) P.cam_pos[a] = cam->position[a];
	P.width = (double)cam->backbuffer_width;
	P.height = (double)cam->backbuffer_height;
	P.inv_width = rmd::exact_reciprocal(P.width), P.inv_height = rmd::exact_reciprocal(P.height);
	P.aspect = P.width / P.height;
	P.tan_half_fov = std::tan(cam->fov_vert / 2.0 * PI / 180.0);
	P.focal_length = cam->focal_length;
	P.aperture_radius = cam->aperture_radius;
	P.W = cam->backbuffer_width, P.H = cam->backbuffer_height;
	P.bounce_limit = st->bounce_limit;
	P.sample_begin = st->sample_begin, P.sample_count = st->sample_count;
	P.n_objects = scene ? scene->n_objects : 0;
	P.n_grids = scene ? scene->n_grids : 0;
	P.mask_words_total = scene ? scene->mask_words_total : 0;
	P.key0 = (uint32_t)st->seed, P.key1 = (uint32_t)(st->seed >> 32);
	P.use_dof = ((st->flags & RMD_RENDER_DOF) && cam->aperture_radius > 0.0) ? 1u : 0u; // off by default, as in the reference's loop (:199)
	// flags 0 = reference-identical: zero-throughput paths are ended only where that provably changes no sample — a scene without grids
	// (its one NaN source, the interpolated normal of a mesh hit, does not exist there); END opts in for scenes with grids, TRACE never ends
	// — AND whose parameters are all inside the class for which that is proved (rmd_scene::regular: an Emission of (inf, 0, 0), a NaN colour, a
	// material of roughness 0 or a sphere of radius 0 make non-finite radiance reachable without a mesh; such a scene is traced like one with a grid)
	// — AND whose camera does not lie on one of its planes (camera_on_a_plane: the view direction of a hit at t = 0 is NaN)
	const bool on_plane = scene && rmd::camera_on_a_plane(scene->planes, cam);
	P.end_black_paths = rmd::end_black_paths_rule(st->flags, scene != nullptr, scene ? scene->n_grids : 0u, scene ? scene->regular : false, on_plane) ? 1u : 0u;
	P.shade_last_depth = (scene && (!scene->regular || on_plane)) ? 1u : 0u;
	P.axis_pairs = scene ? scene->axis_pairs : 0u;
	P.visit_mask = scene ? scene->visit_mask : ~0ull, P.grid_mask = scene ? scene->grid_mask : ~0ull;
	// (bit 1, the tile classes, only where a black bounce is ended: primary_candidates.hpp)
	P.primary_cull = (scene && rmd::primary_cull_allowed(P)) ? (scene->primary_cull & (P.end_black_paths != 0u ? 3u : 1u)) : 0u;
	P.fault = ctx ? ctx->d_fault : nullptr;
	P.walk_batch = rmd::kWalkBatchDefault;
	if (ctx && ctx->tunable[RMD_TUNE_WALK_BATCH] > 0) P.walk_batch = (uint32_t)ctx->tunable[RMD_TUNE_WALK_BATCH]; // any value gives the same image
	// walks put aside for the wave's next walk call (grid_walk.hpp): the carried state is ONE walk's, so only in scenes with one grid object.
	// Low byte: a round's stepping ends under its last K lanes; next byte: a call ends when at most 2K lanes are still walking.
	{
		uint32_t k = rmd::kWalkCutDefault;
		if (ctx && ctx->tunable[RMD_TUNE_WALK_CUT] > 0) k = (uint32_t)std::min<int64_t>(ctx->tunable[RMD_TUNE_WALK_CUT] - 1, 31); // any value gives the same image
		P.walk_cut = (scene && scene->n_grid_objects == 1u) ? (k | (2u * k) << 8) : 0u;
		P.walk_steps_bound = scene ? scene->walk_steps_bound : 0u;
	}
#if RMD_DIAG
	if (ctx) P.debug_flags = ctx->debug_flags;
#endif
	return P;
}

} // namespace rmd

// The host side the first-hit passes share (first_hit.hpp): `launch` enqueues the pass's kernel for the launch parameters P on ctx->stream and
// returns the call's status
template <class Launch>
static rmd_status first_hit_call(rmd_context *ctx, const char *name, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                                 const rmd_tile_rect *tiles, uint32_t n_tiles, Launch launch) {
	rmd_settings st = *settings;
	st.bounce_limit = 1u; // ignored: a pass traces the first segment, and rmd_render_ao one more whatever the limit
	{
		const char *why = nullptr;
		if (!rmd::denoise_rects_ok(tiles, n_tiles, camera->backbuffer_width, camera->backbuffer_height, &why))
			return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, std::string(name) + ": " + why);
	}
	if (rmd_status s = bind(ctx)) return s;
	if (rmd_status s = check_render_args(ctx, scene, camera, &st)) return s;
	if (rmd_status s = prepare_wave_tiles(ctx, camera, tiles, n_tiles)) return s;
	rmd::RenderParams P = rmd::make_params(ctx, scene, camera, &st);
	P.n_work = ctx->n_wave_tiles;
	// (neither the context's events nor its launch record are touched: rmd_last_kernel_ms / rmd_last_launch_info keep describing the last render)
	return launch(P);
}

extern "C" {

uint32_t rmd_abi_version(void) { return RMD_ABI_VERSION; }

rmd_status rmd_context_create(int32_t device_ordinal, rmd_context **out) { return context_create(device_ordinal, nullptr, true, out); }

rmd_status rmd_context_create_on_stream(int32_t device_ordinal, void *hip_stream, rmd_context **out) {
	return context_create(device_ordinal, (hipStream_t)hip_stream, false, out);
}

// The device is selected and both streams are waited for here, in the body: the member buffers are freed after it, and no block may go while a
// stream can still use it.  (A context whose own stream was never created has nothing to wait for.)
rmd_context::~rmd_context() {
	(void)hipSetDevice(device);
	if (stream || !owns_stream) (void)hipStreamSynchronize(stream);
	if (h_fault) (void)hipHostFree(h_fault);
	if (copy_stream) (void)hipStreamSynchronize(copy_stream);
	for (auto &sl : transfer) {
		if (sl.packed_ready) (void)hipEventDestroy(sl.packed_ready);
		if (sl.copied) (void)hipEventDestroy(sl.copied);
	}
	if (copy_stream) (void)hipStreamDestroy(copy_stream);
	if (ev_start) (void)hipEventDestroy(ev_start);
	if (ev_stop) (void)hipEventDestroy(ev_stop);
	if (owns_stream && stream) (void)hipStreamDestroy(stream);
}

void rmd_context_destroy(rmd_context *ctx) { delete ctx; }

const char *rmd_last_error(const rmd_context *ctx) { return ctx ? ctx->last_error.c_str() : tl_last_error.c_str(); }

// A work item is (wave tile, sample range): a tile's samples are split over K items whose waves store per-sample radiance to an HBM
// scratch buffer, added to the pixels in sample order afterwards (by the wave that finishes a tile last, or by sum_kernel) — bit-identical
// to the unsplit launch (tests/test_gpu_parity.py::test_sample_split_is_bit_exact).  It buys enough items to level the launch over 256 CUs
// when wave tiles are few (an N-way shard) or very uneven (a mesh), and lanes that draw (pixel, sample) pairs from the item's pool instead
// of idling until the tile's longest pixel is done.  RMD_TUNE_SAMPLE_SPLIT forces K.  In automatic mode the persistent launches of the spheres kernel
// split only the END of their list this way and run the tiles before it as one item each (plan_work_list below): K is then the tail's.
// `buffered` (out): whether the launch runs the tiles-buffered instantiation.  A split launch (K > 1) always does; a launch too short to split
// does too — as ONE item per wave tile — in scenes with grids (the direct instantiation of the mesh kernel is the slower one at any size: C3 at
// 4 spp 5.6 ms direct, 4.5 ms as two items of 2 samples; progressive passes of a host scheduler are such launches) and, from kSortedMinSamples
// samples on, in scenes without.  RMD_TUNE_SAMPLE_SPLIT = 1 still forces the direct mode (the scratch-free route).
static uint32_t choose_split(const rmd_context *ctx, bool has_grid, uint32_t n_wave_tiles, uint32_t sample_count, bool *buffered = nullptr) {
	uint32_t k = 1;
	bool may_buffer_unsplit = n_wave_tiles != 0 && sample_count >= (has_grid ? 1u : rmd::kSortedMinSamples);
	if (ctx->tunable[RMD_TUNE_SAMPLE_SPLIT] > 0) {
		k = (uint32_t)ctx->tunable[RMD_TUNE_SAMPLE_SPLIT];
		if (k > sample_count / 4u) k = sample_count / 4u; // a forced split keeps >= 4 samples (256 pool items) per wave
		may_buffer_unsplit = false;
	} else if (n_wave_tiles != 0) {
		// Mesh kernel: about 64 work items per wave slot level the tail of a launch of persistent workgroups (tools/split_sweep.py — full C3 frame:
		// 512.8 ms at 32, 508.1 at 64 .. 128, 517.8 at 500), of at least 4 samples each.  Spheres kernel (trips sorted by role,
		// render_kernel.hpp): an item ends with a few ever emptier trips while its last paths finish, a release and, for a tile's last item, the
		// ordered sum, so its items are larger — about 24 per wave slot, at least 64 samples each (round 4, full C2 frame: 52.9 ms at 3 .. 6
		// items per wave tile, 55.2 at 9, 59.1 at 12; an N-way tile share, tools/shard_split.py: N = 8 7.4 ms at 7 .. 10, 8.5 at 16, 9.2 at 3;
		// N = 2 27.3 at 6 .. 7, 29.0 at 2, 29.8 at 12)
		const uint32_t waves_per_slot = has_grid ? 256u : 24u; // (grid scenes: 64 until the work items were chained — an item's end costs a chaining wave nothing, and smaller items even the launch's tail out: C3 382.8 ms at 9 items per wave tile, 381.3 at 32, 381.0 at 64)
		k = (waves_per_slot * ctx->wave_slots + n_wave_tiles - 1u) / n_wave_tiles;
		if (has_grid && k < 2u) k = 2u; // the mesh kernel's direct instantiation is the slower one at any size
		// (launches short enough for the instantiation whose waves chain their work items — an item's end costs them nothing — take items of 2)
		uint32_t min_samples = has_grid ? (sample_count <= rmd::kChainMaxSamples && ctx->tunable[RMD_TUNE_CHAIN_ITEMS] != 1 ? 2u : rmd::kSplitMinSamplesGrid) : 64u;
		if (ctx->tunable[RMD_TUNE_SPLIT_MIN_SAMPLES] > 0) min_samples = (uint32_t)std::min<int64_t>(ctx->tunable[RMD_TUNE_SPLIT_MIN_SAMPLES], 1 << 20);
		if (k > sample_count / min_samples) k = sample_count / min_samples;
		// ... but two items per wave tile while each still holds two samples (C3 at 4 spp: 4.5 ms as two items of 2 samples, 5.1 as one item of 4:
		// with one item per wave tile the mesh tiles' items are the launch's tail)
		if (has_grid && k < 2u && sample_count >= 4u && ctx->tunable[RMD_TUNE_SPLIT_MIN_SAMPLES] <= 0) k = 2u;
	}
	if (k > 64u) k = 64u;
	while (k > 1u && (uint64_t)n_wave_tiles * k > 0x7FFFFFFFull) k--; // work items are indexed in 32 bits
	if (k < 2u) k = 1u;
	if (buffered) *buffered = k > 1u || may_buffer_unsplit;
	return k;
}

extern "C++" {
namespace rmd {
// The spheres kernel's work list (work_list.hpp): which wave tiles run as ONE item.  What an item costs beside its samples — a drain of its last <= 168
// parked hits in ever smaller trips, the tile's candidate set (about 1,270 instructions), an agent-scope release that writes back the XCD's L2, an
// atomic, and a wave that issues nothing meanwhile — buys an even END of the launch and nothing before it.  So the tail of the list alone is split:
//   n_tail   = tail_x2 / 2 wave tiles per wave slot (kTailTilesPerSlotX2: c = 2.5), the LAST tiles of the list; a list with no more tiles than that (an
//              8-way tile share, a small frame) is all tail and the launch is the uniform split it always was;
//   k_tail   = the uniform rule's k (k_uniform: choose_split), or tail_parts (kTailParts = 4) where that is more and every part keeps min_samples samples;
//   n_whole  = the other tiles, first in the list, all samples of the pass each.
// Why 2.5: a whole item cannot be divided, so the one that starts LAST must end before the tail does — the tail has to last as long as the list's
// longest tile takes, and on C2 a tile through the spheres takes about 2.5 times the mean tile.  A shorter tail works only while the long tiles
// happen to lie early in the list.  Measured with tools/work_list_sweep.py, C2 at 500 spp, kernel ms, c = 0 (uniform) / 1 / 1.5 / 2 / 2.5 / 3 —
//   full frame (7.9 tiles a slot)   40.6 / 39.7 / 39.1 .. 39.6 / 39.1 .. 39.4 / 39.0 .. 39.1 / 39.2 .. 39.5   (k_tail 3 .. 5 alike, 6 and 7 up to 1.5 ms slower)
//   2-way share (4.0)               23.1 / 23.1 / 23.3 / 21.0 / 21.3 / 21.9        3-way (2.6)  15.5 / 16.9 / 16.4 / 14.5 / 15.0 / all tail
//   4-way share (2.0)               11.6 / 13.7 / 11.0 / all tail from 2 on        8-way: all tail at every c; at 200 spp 19.0 / - / 16.3 / 16.7 / 16.9 / 17.0
// — at c = 1 and 1.5 the shares whose long tiles start late (2-, 3-, 4-way) are no faster or up to 18 % SLOWER than the uniform split; from 2 on none is.
// Whole items are planned only for passes of at most kWholeMaxSamples = 2^20 samples (a whole item's pool indices, sample_count x 64 < 2^26, and its
// trip bound keep six bits of room in their 32-bit fields).  n_tail_forced (DIAG builds: RMD_DEBUG bit 1024): a tail of that many tiles whatever the slots.
WorkPlan plan_work_list(uint32_t wave_slots, uint32_t n_tiles, uint32_t sample_count, uint32_t k_uniform, uint32_t min_samples, uint32_t tail_x2, uint32_t tail_parts,
                        uint32_t n_tail_forced) {
	WorkPlan w{0u, n_tiles, k_uniform < 1u ? 1u : k_uniform};
	if (tail_x2 == 0u || sample_count > kWholeMaxSamples) return w;
	const uint64_t n_tail = n_tail_forced ? (uint64_t)n_tail_forced : ((uint64_t)tail_x2 * wave_slots + 1u) / 2u;
	if ((uint64_t)n_tiles <= n_tail) return w; // few tiles: everything is tail
	uint32_t k = tail_parts > 64u ? 64u : tail_parts;
	if (min_samples < 1u) min_samples = 1u;
	if (k > sample_count / min_samples) k = sample_count / min_samples;
	if (k < w.k_tail) k = w.k_tail;
	if ((uint64_t)(n_tiles - n_tail) + n_tail * k > 0x7FFFFFFFull) return w; // work items are indexed in 32 bits (never: n_tail * 64 < 2^31 - n_tiles for any device)
	w.n_whole = n_tiles - (uint32_t)n_tail, w.n_tail = (uint32_t)n_tail, w.k_tail = k;
	return w;
}
// One pass's list: the uniform split of choose_split, and for a buffered persistent pass of a scene without grids in automatic mode the two-part
// list.  A forced RMD_TUNE_SAMPLE_SPLIT, the one-wave-per-item form and every scene with grids keep the uniform split (n_whole = 0).
static WorkPlan pass_work_plan(const rmd_context *ctx, bool has_grid, bool split_launch, bool buffered, bool persistent, uint32_t n_tiles, uint32_t sample_count,
                               bool *persistent_pass) {
	WorkPlan w{0u, n_tiles, split_launch ? choose_split(ctx, has_grid, n_tiles, sample_count) : 1u};
	// (a launch with fewer work items than the device has wave slots spreads better as one wave per item)
	*persistent_pass = persistent && ((uint64_t)n_tiles * w.k_tail >= ctx->wave_slots || ctx->tunable[RMD_TUNE_LAUNCH_FORM] == 2);
	if (!buffered || has_grid || !*persistent_pass || ctx->tunable[RMD_TUNE_SAMPLE_SPLIT] > 0) return w;
	uint32_t min_samples = kTailMinSamples, forced_tail = 0u;
	if (ctx->tunable[RMD_TUNE_SPLIT_MIN_SAMPLES] > 0) min_samples = (uint32_t)std::min<int64_t>(ctx->tunable[RMD_TUNE_SPLIT_MIN_SAMPLES], 1 << 20);
#if RMD_DIAG
	if (ctx->debug_flags & 1024u) forced_tail = 4u; // both kinds of item in a frame of a few dozen wave tiles (tests/test_gpu_whole_tile_items.py)
#endif
	return plan_work_list(ctx->wave_slots, n_tiles, sample_count, w.k_tail, min_samples, ctx->tail_x2, ctx->tail_parts, forced_tail);
}
// the list this context gives a pass of pass_samples samples of a render of n_tiles wave tiles and sample_count samples, provided the scratch for the
// render's passes can be had (probe.cpp: rmd_probe_work_plan) — the render decides whether it is buffered, the pass its own list
WorkPlan context_work_plan(const rmd_context *ctx, bool has_grid, uint32_t n_tiles, uint32_t sample_count, uint32_t pass_samples) {
	bool buffered = false, persistent_pass = false;
	const uint32_t split = choose_split(ctx, has_grid, n_tiles, sample_count, &buffered);
	return pass_work_plan(ctx, has_grid, split > 1u, buffered, ctx->tunable[RMD_TUNE_LAUNCH_FORM] != 1, n_tiles, pass_samples, &persistent_pass);
}
} // namespace rmd
} // extern "C++"

// Samples per pass of a split launch: the scratch buffer holds n_wave_tiles x 64 x samples x 32 bytes (the whole C3 frame at 500 spp
// is 33 GB, one launch).  By default it may take an eighth of the device memory that is free right now (RMD_TUNE_SCRATCH_CAP_MB
// overrides), never less than 8 samples per pass; what does not fit runs as several passes.  The device may still refuse the
// allocation — other contexts, ranks or tenants hold memory, or the cap was set beyond it: the pass is then halved until a buffer
// can be had (the old one stays until a larger one exists), and when not even 8 samples fit the launch runs unsplit (one wave per
// wave tile, no scratch).  Every route gives the same frame bit for bit.
// n_work: the launch's wave tiles.  split and buffered come in as choose_split's and leave as 1 and false where the launch runs unsplit.
static rmd_status size_sample_scratch(rmd_context *ctx, uint32_t n_work, uint32_t sample_count, uint32_t &per_pass, uint32_t &split, bool &buffered) {
	per_pass = sample_count;
	if (!buffered) return RMD_OK;
	const size_t bytes_per_sample = (size_t)n_work * 64u * rmd::kSampleStride * sizeof(double);
	size_t cap;
	if (ctx->tunable[RMD_TUNE_SCRATCH_CAP_MB] > 0) cap = (size_t)ctx->tunable[RMD_TUNE_SCRATCH_CAP_MB] << 20;
	else {
		size_t free_b = 0, total_b = 0;
		RMD_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
		cap = (free_b + ctx->sample_buf.bytes()) / 8; // the buffer this context already holds counts as available to it
	}
	if (bytes_per_sample * per_pass > cap) per_pass = (uint32_t)(cap / bytes_per_sample);
	// (the mesh kernel numbers a pass's 32-byte sectors in 32 bits: render_kernel.hpp, PathId)
	const uint64_t sectors_per_sample = (uint64_t)n_work * 64u;
	if (sectors_per_sample * per_pass > 0xFFFFFFFFull) per_pass = (uint32_t)(0xFFFFFFFFull / sectors_per_sample);
	if (per_pass < 8u) per_pass = 8u;
	if (per_pass > sample_count) per_pass = sample_count;
	// (a frame of more than 2^32 / 8 / 64 = 8.4 M wave tiles — 537 Mpixel — cannot number even the smallest pass's sectors in 32 bits: unsplit, no scratch)
	if (sectors_per_sample * per_pass > 0xFFFFFFFFull) split = 1u, buffered = false, per_pass = sample_count;
	while (buffered && bytes_per_sample * per_pass > ctx->sample_buf.bytes()) {
		rmd::DeviceBuffer fresh; // allocate first: a pass that finally fits the old block runs in it
		const hipError_t e = fresh.alloc(bytes_per_sample * per_pass);
		if (e == hipSuccess) {
			ctx->sample_buf = std::move(fresh);
			break;
		}
		(void)hipGetLastError(); // the failure is handled here: it must not surface at the next launch check
		if (e != hipErrorOutOfMemory) return rmd::fail(ctx, RMD_ERR_HIP, std::string("hipMalloc(sample scratch): ") + hipGetErrorString(e));
		if (per_pass <= 8u) { // not even the smallest pass: render unsplit
			split = 1u, buffered = false, per_pass = sample_count;
			break;
		}
		per_pass = per_pass / 2u < 8u ? 8u : per_pass / 2u;
	}
	return RMD_OK;
}

// Persistent split launches of scenes with grids keep their paths in queues in device memory (render_kernel.hpp: render_wave_queued;
// RMD_TUNE_PATH_QUEUES: 1 = never): kQueuePaths entries on each of a resident wave's two stacks, 192 bytes a path — 49 KB a wave, 200 MB
// for the 4,096 resident waves of an MI355X — allocated at the first launch that wants them.  A device that cannot provide them runs
// the lane-per-path form (render_wave): the same frame bit for bit.
static rmd_status attach_path_queues(rmd_context *ctx, rmd::RenderParams &Q) {
	const size_t wave_bytes = rmd::path_queue_bytes_host(rmd::kQueuePaths), need = wave_bytes * ctx->wave_slots;
	if (ctx->queue_buf.bytes() < need) {
		// RMD_DEBUG bit 256 (DIAG builds; debug_flags is 0 in any other): the device has no memory for the queues — the fallback below
		// (tests/test_gpu_launch_edges.py)
		const hipError_t qe = (ctx->debug_flags & 256u) ? hipErrorOutOfMemory : ctx->queue_buf.grow(need);
		if (qe == hipSuccess) {
			// (zeroed once: a trip's idle lanes read the trip's first entry, never one nobody wrote — but a fresh allocation should not hold another process's data)
			RMD_HIP(ctx, hipMemsetAsync(ctx->queue_buf.as<void>(), 0, need, ctx->stream));
		} else {
			(void)hipGetLastError();
			if (qe != hipErrorOutOfMemory) return rmd::fail(ctx, RMD_ERR_HIP, std::string("hipMalloc(path queues): ") + hipGetErrorString(qe));
		}
	}
	if (ctx->queue_buf.bytes()) Q.queue_buf = ctx->queue_buf.as<unsigned char>(), Q.queue_wave_bytes = (uint32_t)wave_bytes, Q.queue_paths = rmd::kQueuePaths;
	return RMD_OK;
}

// DIAG builds, RMD_DEBUG bits 8 | 16: the launch's event counters or time stamps, downloaded and printed once the launch has ended
static rmd_status print_debug_counters(rmd_context *ctx, uint32_t debug_flags, bool has_grid) {
	unsigned long long h[64];
	RMD_HIP(ctx, hipMemcpyAsync(h, ctx->debug_counters.as<void>(), sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if ((debug_flags & 16u) && ctx->last_launch.queued) {
		static const char *kinds[3] = {"GEN  ", "SHADE", "WALK "};
		for (int k = 0; k < 3; k++)
			std::fprintf(stderr, "[rmd queued stamps, cycles] %s trips=%llu fetch=%llu make_ray=%llu simple=%llu walk=%llu ray_push=%llu classify=%llu stores=%llu\n", kinds[k], h[k * 8 + 7],
			             h[k * 8 + 0], h[k * 8 + 1], h[k * 8 + 2], h[k * 8 + 3], h[k * 8 + 4], h[k * 8 + 5], h[k * 8 + 6]);
		std::fprintf(stderr, "[rmd queued stamps, cycles] inside the walks: init=%llu stepping=%llu entry_wait=%llu scan=%llu (chunk search+load+test)=%llu hits=%llu tail=%llu\n",
		             h[24], h[25], h[26], h[27], h[29], h[30], h[31]);
	} else if (debug_flags & 16u)
		std::fprintf(stderr, "[rmd stamps, cycles] wave_total=%llu next_ray=%llu simple=%llu walk=%llu classify=%llu | walk: init=%llu stepping=%llu entry_wait=%llu scan=%llu (chunk search+load+test)=%llu hits=%llu tail=%llu\n",
		             h[0], h[1], h[2], h[3], h[4], h[8], h[9], h[10], h[11], h[13], h[14], h[15]);
	else
		std::fprintf(stderr, "[rmd debug] walk_calls=%llu walkers=%llu calls_with_walkers=%llu rounds=%llu wave_steps=%llu lane_steps=%llu test_rounds=%llu tests=%llu chunks=%llu | main_iterations=%llu live_lanes=%llu lanes_with_ray=%llu | stepping iterations with <= 4 / 8 / 16 lanes: %llu / %llu / %llu, with <= 8 lanes while tests wait: %llu\n",
		             h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[8], h[9], h[10], h[11], h[12], h[7], h[13], h[14], h[15]);
	if ((debug_flags & 16u) == 0u)
		std::fprintf(stderr, "[rmd debug] sphere pre-test: pairs passed=%llu full chunks=%llu | pairs dropped that pass the reference's test (flag 64; must be 0)=%llu\n", h[17], h[18], h[16]);
	if ((debug_flags & 16u) == 0u && (debug_flags & 512u))
		std::fprintf(stderr, "[rmd debug] primary candidates: lanes checked=%llu sphere turns left out=%llu trips with two axis pairs left out=%llu | cleared spheres that register a hit (must be 0)=%llu closest hits that differ from the full visit's (must be 0)=%llu\n",
		             h[32], h[35], h[36], h[33], h[34]);
	if ((debug_flags & 16u) == 0u && ctx->last_launch.buffered && !has_grid) // (the role-sorted spheres kernel: render_wave_sorted)
		std::fprintf(stderr, "[rmd debug] lobe trips: diffuse trips=%llu diffuse hits shaded=%llu ggx trips=%llu ggx hits shaded=%llu | hits parked: diffuse=%llu ggx=%llu\n", h[37], h[38], h[39],
		             h[40], h[41], h[42]);
	if ((debug_flags & 16u) == 0u && ctx->last_launch.buffered && !has_grid) // (its items' tile classes: primary_candidates.hpp)
		std::fprintf(stderr, "[rmd debug] tile classes: general items=%llu emitter items=%llu black items=%llu | black rounds=%llu cut short=%llu samples ended in pass A=%llu survivors=%llu | samples checked against their full path=%llu that are not what the class says (must be 0)=%llu rays that hit another object than the wall (must be 0)=%llu\n",
		             h[48], h[49], h[50], h[52], h[54], h[51], h[53], h[55], h[56], h[57]);
	if ((debug_flags & 16u) == 0u && ctx->last_launch.queued)
		std::fprintf(stderr, "[rmd debug] path queues: rays pushed=%llu (of them walks put aside=%llu) rays held in their lanes=%llu hits pushed=%llu hits held in their lanes=%llu\n", h[19], h[22], h[23], h[20], h[21]);
	return RMD_OK;
}

static rmd_status render_tiles_async_impl(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                                          const rmd_tile_rect *tiles, uint32_t n_tiles, double *accum_dev, double *accum_sq_dev) {
	if (rmd_status s = bind(ctx)) return s;
	if (rmd_status s = check_render_args(ctx, scene, camera, settings)) return s;
	if (!accum_dev || (n_tiles && !tiles)) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_render_tiles: null tiles/accum pointer");
	if (rmd_status s = prepare_wave_tiles(ctx, camera, tiles, n_tiles)) return s;
	if (settings->bounce_limit == 0u) { // trace(.., 1) with depth 1 > bounce_limit returns (0, 0, 0) unintersected (src/trace.rs:235-237): pixel += 0
		RMD_HIP(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
		RMD_HIP(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
		ctx->timed = true;
		return RMD_OK;
	}
	rmd::RenderParams P = rmd::make_params(ctx, scene, camera, settings);
	P.n_work = ctx->n_wave_tiles;
	if (P.debug_flags & 24u) {
		RMD_HIP(ctx, ctx->debug_counters.grow(64 * sizeof(unsigned long long)));
		RMD_HIP(ctx, hipMemsetAsync(ctx->debug_counters.as<void>(), 0, 64 * sizeof(unsigned long long), ctx->stream));
		P.debug_counters = ctx->debug_counters.as<unsigned long long>();
	}
	bool buffered = false;
	uint32_t split = choose_split(ctx, scene->n_grids != 0, P.n_work, P.sample_count, &buffered);
	// default form: persistent workgroups, one per CU, whose waves draw their work items from a counter (form 1: one wave per work
	// item — round 1's; 4.7 % slower on the benchmark mesh, 2.4 % on the spheres frame, where a workgroup launch per item cost ~100 us
	// of a wave slot each: 152 vs 113.6 ms at 32 items per wave tile)
	const bool persistent = ctx->tunable[RMD_TUNE_LAUNCH_FORM] != 1;
	if (persistent) RMD_HIP(ctx, ctx->work_counter.grow(256));
	uint32_t per_pass = 0;
	if (rmd_status s = size_sample_scratch(ctx, P.n_work, P.sample_count, per_pass, split, buffered)) return s;
	ctx->last_launch = rmd_launch_info{};
	ctx->last_launch.end_black_paths = P.end_black_paths, ctx->last_launch.has_grid = scene->n_grids != 0u;
	RMD_HIP(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
	for (uint64_t done = 0; done < settings->sample_count || done == 0; done += per_pass) { // 64-bit: sample_count may be close to 2^32
		rmd::RenderParams Q = P;
		Q.sample_begin = settings->sample_begin + (uint32_t)done;
		Q.sample_count = settings->sample_count - done < per_pass ? (uint32_t)(settings->sample_count - done) : per_pass;
		bool persistent_pass = false;
		const rmd::WorkPlan list = rmd::pass_work_plan(ctx, scene->n_grids != 0, split > 1u, buffered, persistent, P.n_work, Q.sample_count, &persistent_pass);
		Q.split_k = list.k_tail, Q.n_whole = list.n_whole;
		Q.sample_magic = Q.sample_count > 1u ? ~0ull / Q.sample_count + 1ull : 0ull; // floor(2^64 / d) + 1 for d >= 2 (2^64 - 1 and 2^64 have the same quotient unless d divides 2^64: then + 1 overshoots by one and is still exact for dividends below 2^32)
		Q.buffered = buffered ? 1u : 0u;
		{ // split launches of grid scenes chain their work items (launch.hpp: kChainMaxSamples; RMD_TUNE_CHAIN_ITEMS: 1 = never, 2 = always)
			const int64_t force = ctx->tunable[RMD_TUNE_CHAIN_ITEMS];
			Q.chain_items = (buffered && scene->n_grids != 0u && (force == 2 || (force == 0 && Q.sample_count <= rmd::kChainMaxSamples))) ? 1u : 0u;
		}
		Q.sample_buf = ctx->sample_buf.as<double>();
		if (persistent_pass) {
			RMD_HIP(ctx, hipMemsetAsync(ctx->work_counter.as<void>(), 0, sizeof(uint32_t), ctx->stream));
			Q.work_counter = ctx->work_counter.as<uint32_t>();
		}
		if (persistent_pass && buffered && scene->n_grids != 0u && ctx->tunable[RMD_TUNE_PATH_QUEUES] != 1)
			if (rmd_status s = attach_path_queues(ctx, Q)) return s;
		// spheres kernel: the wave that finishes a wave tile last adds the tile's samples to the pixels itself (no second kernel: 120.3 ->
		// 117.0 ms per C2 frame).  Mesh scenes keep sum_kernel: their kernel waits on memory a third of the time, and the sum's 33 GB of
		// streaming reads in between cost it more (491.4 vs 487.3 ms on C3) than the separate kernel's 5.5 ms
		if (buffered && scene->n_grids == 0) {
			RMD_HIP(ctx, ctx->tile_done.grow((size_t)P.n_work * sizeof(uint32_t)));
			RMD_HIP(ctx, hipMemsetAsync(ctx->tile_done.as<void>(), 0, (size_t)P.n_work * sizeof(uint32_t), ctx->stream));
			Q.tile_done = ctx->tile_done.as<uint32_t>();
		}
		rmd::LaunchShape shape;
		RMD_HIP(ctx, rmd::launch_render_tiles(ctx->stream, Q, scene->d_objects, scene->d_grids, ctx->wave_tiles.as<rmd::WaveTile>(), accum_dev, persistent_pass ? ctx->n_cus : 0u, &shape,
		                                      accum_sq_dev));
		ctx->last_launch.passes++, ctx->last_launch.split_k = Q.split_k, ctx->last_launch.buffered = Q.buffered;
		ctx->last_launch.persistent = shape.persistent, ctx->last_launch.waves_per_workgroup = shape.waves_per_wg; // the form it was launched in, not the one asked for
		ctx->last_launch.queued = shape.queued;
		ctx->last_launch.chained = shape.chained;
		if (settings->sample_count == 0) break;
	}
	RMD_HIP(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
	ctx->timed = true;
	if (P.debug_flags & 24u) return print_debug_counters(ctx, P.debug_flags, scene->n_grids != 0u);
	return RMD_OK;
}

rmd_status rmd_render_tiles_async(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                                  const rmd_tile_rect *tiles, uint32_t n_tiles, double *accum_dev) {
	// (the wave-tile table and the cached rectangle list are std::vectors: nothing throws across the boundary)
	return rmd::guarded(ctx, "rmd_render_tiles", [&] { return render_tiles_async_impl(ctx, scene, camera, settings, tiles, n_tiles, accum_dev, nullptr); });
}

rmd_status rmd_render_tiles_moments_async(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                                          const rmd_tile_rect *tiles, uint32_t n_tiles, double *accum_dev, double *accum_sq_dev) {
	if (accum_sq_dev != nullptr && accum_sq_dev == accum_dev)
		return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_render_tiles_moments: accum_sq_dev must not alias accum_dev");
	return rmd::guarded(ctx, "rmd_render_tiles_moments",
	                    [&] { return render_tiles_async_impl(ctx, scene, camera, settings, tiles, n_tiles, accum_dev, accum_sq_dev); });
}

rmd_status rmd_context_set_tunable(rmd_context *ctx, uint32_t key, int64_t value) {
	if (!ctx) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "rmd_context_set_tunable: null context");
	if (key >= RMD_TUNE_COUNT || value < 0) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_context_set_tunable: unknown key or negative value");
	if (key == RMD_TUNE_LAUNCH_FORM && value > 2) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_context_set_tunable: launch form is 0 .. 2");
	ctx->tunable[key] = value;
	return RMD_OK;
}
rmd_status rmd_context_get_tunable(const rmd_context *ctx, uint32_t key, int64_t *out_value) {
	if (!ctx || !out_value || key >= RMD_TUNE_COUNT) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "rmd_context_get_tunable: bad argument");
	*out_value = ctx->tunable[key];
	return RMD_OK;
}

rmd_status rmd_context_memory_info(rmd_context *ctx, uint64_t *out_free_bytes, uint64_t *out_total_bytes) {
	if (rmd_status s = bind(ctx)) return s;
	if (!out_free_bytes || !out_total_bytes) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_context_memory_info: null pointer");
	size_t free_b = 0, total_b = 0;
	RMD_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
	*out_free_bytes = free_b, *out_total_bytes = total_b;
	return RMD_OK;
}

rmd_status rmd_context_synchronize(rmd_context *ctx) {
	if (rmd_status s = bind(ctx)) return s;
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return rmd::check_fault(ctx);
}

rmd_status rmd_render_tiles(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                            const rmd_tile_rect *tiles, uint32_t n_tiles, double *accum_dev) {
	if (rmd_status s = rmd_render_tiles_async(ctx, scene, camera, settings, tiles, n_tiles, accum_dev)) return s;
	return rmd_context_synchronize(ctx);
}

rmd_status rmd_render_tiles_moments(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                                    const rmd_tile_rect *tiles, uint32_t n_tiles, double *accum_dev, double *accum_sq_dev) {
	if (rmd_status s = rmd_render_tiles_moments_async(ctx, scene, camera, settings, tiles, n_tiles, accum_dev, accum_sq_dev)) return s;
	return rmd_context_synchronize(ctx);
}



rmd_status rmd_render_features_async(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                                     const rmd_tile_rect *tiles, uint32_t n_tiles, double *feat_dev, double *feat_sq_dev) {
	if (!scene || !camera || !settings) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_render_features: null scene/camera/settings");
	if (!feat_dev || (n_tiles && !tiles)) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_render_features: null tiles/feat pointer");
	// the two W*H*7-double ranges must not overlap
	const unsigned __int128 bytes = (unsigned __int128)camera->backbuffer_width * camera->backbuffer_height * RMD_FEATURE_CHANNELS * sizeof(double);
	if (rmd::any_overlap({{feat_dev, bytes}, {feat_sq_dev, bytes}})) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_render_features: feat_sq_dev must not alias feat_dev");
	return rmd::guarded(ctx, "rmd_render_features", [&] {
		return first_hit_call(ctx, "rmd_render_features", scene, camera, settings, tiles, n_tiles, [&](const rmd::RenderParams &P) -> rmd_status {
			RMD_HIP(ctx, rmd::launch_features(ctx->stream, P, scene->d_objects, scene->d_grids, ctx->wave_tiles.as<rmd::WaveTile>(), feat_dev, feat_sq_dev));
			return RMD_OK;
		});
	});
}

rmd_status rmd_render_features(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                               const rmd_tile_rect *tiles, uint32_t n_tiles, double *feat_dev, double *feat_sq_dev) {
	if (rmd_status s = rmd_render_features_async(ctx, scene, camera, settings, tiles, n_tiles, feat_dev, feat_sq_dev)) return s;
	return rmd_context_synchronize(ctx);
}

// First-hit object IDs (ids.hip): rmd_render_features' host side with the ID buffer in place of the two feature buffers
rmd_status rmd_render_ids_async(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings, const rmd_tile_rect *tiles,
                                uint32_t n_tiles, uint32_t *ids_dev) {
	if (!scene || !camera || !settings) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_render_ids: null scene/camera/settings");
	if (!ids_dev || (n_tiles && !tiles)) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_render_ids: null tiles/ids pointer");
	return rmd::guarded(ctx, "rmd_render_ids", [&] {
		return first_hit_call(ctx, "rmd_render_ids", scene, camera, settings, tiles, n_tiles, [&](const rmd::RenderParams &P) -> rmd_status {
			RMD_HIP(ctx, rmd::launch_ids(ctx->stream, P, scene->d_objects, scene->d_grids, ctx->wave_tiles.as<rmd::WaveTile>(), ids_dev));
			return RMD_OK;
		});
	});
}

rmd_status rmd_render_ids(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings, const rmd_tile_rect *tiles,
                          uint32_t n_tiles, uint32_t *ids_dev) {
	if (rmd_status s = rmd_render_ids_async(ctx, scene, camera, settings, tiles, n_tiles, ids_dev)) return s;
	return rmd_context_synchronize(ctx);
}

// The matte of a set of objects from an ID buffer.  The refusals in the header's order, the context last.  The block: [counter: 16 bytes][keys]
rmd_status rmd_ids_matte(rmd_context *ctx, const uint32_t *ids_dev, uint32_t width, uint32_t height, const uint32_t *objects, uint32_t n_objects, double *matte_dev,
                         uint64_t *other_pixels_host) {
	return rmd::guarded(ctx, "rmd_ids_matte", [&]() -> rmd_status {
		const std::string name = "rmd_ids_matte: ";
		if (width == 0 || height == 0) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, name + "width or height is 0");
		if (!ids_dev || !matte_dev) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, name + "null ids/matte pointer");
		if (n_objects && !objects) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, name + "null objects with n_objects > 0");
		if (n_objects > rmd::kIdsMatteMaxObjects) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, name + "more than 2048 objects");
		std::vector<uint32_t> keys(n_objects);
		for (uint32_t i = 0; i < n_objects; i++) {
			if (objects[i] == RMD_ID_MISS - 1u) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, name + "object index 0xFFFFFFFE: its key would be RMD_ID_MISS");
			keys[i] = rmd::ids_key_of(objects[i]);
		}
		const unsigned __int128 n = (unsigned __int128)width * height;
		if (rmd::any_overlap({{ids_dev, n * RMD_ID_WORDS * sizeof(uint32_t)}, {matte_dev, n * sizeof(double)}}))
			return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, name + "matte_dev overlaps ids_dev");
		if (rmd_status s = bind(ctx)) return s;
		std::sort(keys.begin(), keys.end());
		keys.erase(std::unique(keys.begin(), keys.end()), keys.end()); // duplicates are allowed: it is a set
		RMD_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the call waits for the frame's passes in any case: the keys go up on an idle stream, from pageable memory
		RMD_HIP(ctx, ctx->ids_matte_scratch.grow(16 + (size_t)rmd::kIdsMatteMaxObjects * sizeof(uint32_t)));
		unsigned long long *d_other = ctx->ids_matte_scratch.as<unsigned long long>();
		uint32_t *d_keys = reinterpret_cast<uint32_t *>(ctx->ids_matte_scratch.as<unsigned char>() + 16);
		RMD_HIP(ctx, hipMemsetAsync(d_other, 0, 16, ctx->stream));
		if (!keys.empty()) RMD_HIP(ctx, hipMemcpyAsync(d_keys, keys.data(), keys.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
		RMD_HIP(ctx, rmd::launch_ids_matte(ctx->stream, ids_dev, (uint64_t)width * height, d_keys, (uint32_t)keys.size(), matte_dev, d_other));
		unsigned long long other = 0;
		RMD_HIP(ctx, hipMemcpyAsync(&other, d_other, sizeof(other), hipMemcpyDeviceToHost, ctx->stream));
		RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
		if (other_pixels_host) *other_pixels_host = other;
		return rmd::check_fault(ctx);
	});
}

// Ambient occlusion of the first hit (ao.hip): rmd_render_ids' host side with max_distance checked in front of first_hit_call's own refusals
rmd_status rmd_render_ao_async(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings, const rmd_tile_rect *tiles,
                               uint32_t n_tiles, double max_distance, uint32_t *ao_dev) {
	if (!scene || !camera || !settings) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_render_ao: null scene/camera/settings");
	if (!ao_dev || (n_tiles && !tiles)) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_render_ao: null tiles/ao pointer");
	if (!(max_distance > 0.0)) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_render_ao: max_distance must be > 0"); // (NaN: refused; +inf: any hit)
	return rmd::guarded(ctx, "rmd_render_ao", [&] {
		return first_hit_call(ctx, "rmd_render_ao", scene, camera, settings, tiles, n_tiles, [&](const rmd::RenderParams &P) -> rmd_status {
			RMD_HIP(ctx, rmd::launch_ao(ctx->stream, P, scene->d_objects, scene->d_grids, ctx->wave_tiles.as<rmd::WaveTile>(), ao_dev, max_distance));
			return RMD_OK;
		});
	});
}

rmd_status rmd_render_ao(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings, const rmd_tile_rect *tiles,
                         uint32_t n_tiles, double max_distance, uint32_t *ao_dev) {
	if (rmd_status s = rmd_render_ao_async(ctx, scene, camera, settings, tiles, n_tiles, max_distance, ao_dev)) return s;
	return rmd_context_synchronize(ctx);
}

// The openness of every pixel from an AO buffer.  The refusals in the header's order, the context last.  The block: [counter: 16 bytes]
rmd_status rmd_ao_resolve(rmd_context *ctx, const uint32_t *ao_dev, uint32_t width, uint32_t height, double empty_value, double *out_dev, uint64_t *empty_pixels_host) {
	return rmd::guarded(ctx, "rmd_ao_resolve", [&]() -> rmd_status {
		const std::string name = "rmd_ao_resolve: ";
		if (width == 0 || height == 0) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, name + "width or height is 0");
		if (!ao_dev || !out_dev) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, name + "null ao/out pointer");
		if (!std::isfinite(empty_value)) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, name + "empty_value is not finite");
		const unsigned __int128 n = (unsigned __int128)width * height;
		if (rmd::any_overlap({{ao_dev, n * RMD_AO_WORDS * sizeof(uint32_t)}, {out_dev, n * sizeof(double)}}))
			return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, name + "out_dev overlaps ao_dev");
		if (rmd_status s = bind(ctx)) return s;
		RMD_HIP(ctx, ctx->ao_resolve_scratch.grow(16));
		unsigned long long *d_empty = ctx->ao_resolve_scratch.as<unsigned long long>();
		RMD_HIP(ctx, hipMemsetAsync(d_empty, 0, 16, ctx->stream));
		RMD_HIP(ctx, rmd::launch_ao_resolve(ctx->stream, ao_dev, (uint64_t)width * height, empty_value, out_dev, d_empty));
		unsigned long long empty = 0;
		RMD_HIP(ctx, hipMemcpyAsync(&empty, d_empty, sizeof(empty), hipMemcpyDeviceToHost, ctx->stream));
		RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
		if (empty_pixels_host) *empty_pixels_host = empty;
		return rmd::check_fault(ctx);
	});
}

rmd_status rmd_render_tiles_host(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                                 const rmd_tile_rect *tiles, uint32_t n_tiles, double *accum_host) {
	if (rmd_status s = bind(ctx)) return s;
	if (!camera || !accum_host) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_render_tiles_host: null argument");
	size_t n = (size_t)camera->backbuffer_width * camera->backbuffer_height * 3;
	rmd::DeviceBuffer dev;
	RMD_HIP(ctx, dev.alloc(n * sizeof(double)));
	rmd_status s = rmd_framebuffer_upload(ctx, accum_host, dev.as<double>(), n);
	if (!s) s = rmd_render_tiles(ctx, scene, camera, settings, tiles, n_tiles, dev.as<double>());
	if (!s) s = rmd_framebuffer_download(ctx, dev.as<double>(), accum_host, n);
	return s;
}


rmd_status rmd_host_alloc(rmd_context *ctx, size_t bytes, void **out_host) {
	if (rmd_status s = bind(ctx)) return s;
	if (!out_host || bytes == 0) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_host_alloc: bad argument");
	*out_host = nullptr;
	RMD_HIP(ctx, hipHostMalloc(out_host, bytes, hipHostMallocDefault));
	return RMD_OK;
}
rmd_status rmd_host_free(rmd_context *ctx, void *host) { // (ctx may be NULL: a block may outlive the context it was allocated through)
	if (ctx)
		if (rmd_status s = bind(ctx)) return s;
	if (host) RMD_HIP(ctx, hipHostFree(host));
	return RMD_OK;
}

rmd_status rmd_last_kernel_ms(rmd_context *ctx, float *out_ms) {
	if (rmd_status s = bind(ctx)) return s;
	if (!out_ms) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_last_kernel_ms: null pointer");
	if (!ctx->timed) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_last_kernel_ms: no render has been enqueued on this context");
	RMD_HIP(ctx, hipEventSynchronize(ctx->ev_stop));
	RMD_HIP(ctx, hipEventElapsedTime(out_ms, ctx->ev_start, ctx->ev_stop));
	return rmd::check_fault(ctx);
}

rmd_status rmd_last_launch_info(const rmd_context *ctx, rmd_launch_info *out) {
	if (!ctx || !out) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "rmd_last_launch_info: null argument");
	*out = ctx->last_launch;
	return RMD_OK;
}


} // extern "C"
