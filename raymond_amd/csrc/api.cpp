// C-ABI implementation (include/raymond_hip.h): contexts, scene upload, the render entry points,
// framebuffer helpers and the resolve/tone-map epilogue (the denoise entry points: api_denoise.cpp).  Host code only; kernels are in kernels.hip.
#define RMD_WITH_HIP 1
#include <algorithm>
#include <cmath>
#include <limits>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "internal.hpp"
#include "launch.hpp"
#include "luma_bins.hpp"
#include "resolve_tiles_host.hpp"

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
		if (r.width == 0 || r.height == 0) continue;
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

// What rmd_scene_create derives from a grid description before it uploads it (device_types.hpp: DevGrid): validated tables, the triangle
// records, the per-cell index lists with their entries, the Heron constants.  ~50 ms of host time for the 99k-triangle benchmark mesh — a host
// scheduler creates a scene per render_tiled call and per GPU (the counterpart of the reference's per-worker `scene.clone()`, src/trace.rs:182-185),
// so a description that comes from a rmd_grid_build (rmd_grid_desc::built) keeps them in that object: derived once, shared by every upload.
struct GridDerived {
	std::vector<unsigned char> recs;
	std::vector<rmd::CellEntry> entries;
	std::vector<uint32_t> ids;
	std::vector<double> aux;
	std::vector<double> spheres; // per triangle: centre and squared radius of a sphere around it, inflated (device_types.hpp: DevGrid::tri_sph)
	double sphere_kb = 0.0;      // ... and the grid's distance-proportional allowance (DevGrid::sph_kb)
};
static rmd_status derive_grid_tables(rmd_context *ctx, const rmd_grid_desc &g, GridDerived &out) {
	{
		if (!g.cells || !g.mapping_table || !g.tri_pos || !g.tri_nrm || g.n_tris == 0 ||
		    g.n_cells != (uint64_t)g.resolution[0] * g.resolution[1] * g.resolution[2]) {
			return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_scene_create: inconsistent grid description");
		}
		// validate the CSR-like table so that the kernel's gathers stay in bounds
		for (uint64_t c = 0; c < g.n_cells; c++) {
			uint64_t off = g.cells[c];
			if (off >= g.n_mapping || off + (uint64_t)g.mapping_table[off] >= g.n_mapping) {
				return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_scene_create: cells/mapping_table run out of range");
			}
			uint32_t cnt = g.mapping_table[off];
			for (uint32_t k = 1; k <= cnt; k++)
				if (g.mapping_table[off + k] >= g.n_tris) {
					return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_scene_create: triangle index out of range in mapping_table");
				}
		}
		// the kernel keeps the reference's linear cell index x + res.x*(y + z*res.z) in 32 bits
		if ((uint64_t)g.resolution[0] * ((uint64_t)g.resolution[1] + (uint64_t)g.resolution[2] * g.resolution[2]) >= (1ull << 31) ||
		    g.n_cells > (1ull << 31)) {
			return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "rmd_scene_create: grid resolution too large for 31-bit cell indices");
		}
		// triangle records, per-cell lists of triangle indices and the cell entries (device_types.hpp): record = v0, edge1 = v1 - v0,
		// edge2 = v2 - v0 (triangle.rs:16-17, same subtraction, done once); entry slot 0 = the cell's list in mapping_table order, slots 1..6 =
		// that list without the triangles the cell at index c - delta_s lists too (the cell a walk came from: tested already, missed)
		const uint64_t n_refs = g.n_mapping - g.n_cells;
		if (n_refs > 0xFFFFFFFFull) {
			return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "rmd_scene_create: more than 2^32-1 cell->triangle references");
		}
		std::vector<unsigned char> &recs = out.recs;
		recs.assign((size_t)g.n_tris * rmd::kTriRecStride, 0);
		for (uint64_t ti = 0; ti < g.n_tris; ti++) {
			const double *p = g.tri_pos + (size_t)ti * 9;
			double q[9];
			for (int a = 0; a < 3; a++) q[a] = p[a], q[3 + a] = p[3 + a] - p[a], q[6 + a] = p[6 + a] - p[a];
			std::memcpy(recs.data() + (size_t)ti * rmd::kTriRecStride, q, sizeof(q));
		}
		std::vector<rmd::CellEntry> &entries = out.entries;
		entries.assign((size_t)g.n_cells * rmd::kEntrySlots, rmd::CellEntry{0u, 0u});
		std::vector<uint32_t> &ids = out.ids;
		ids.clear();
		ids.reserve((size_t)n_refs * 3);
		{
			uint64_t refs_seen = 0;
			for (uint64_t c = 0; c < g.n_cells; c++) { // slot 0: the full lists, validated against overlapping runs
				const uint32_t off = g.cells[c], cnt = g.mapping_table[off];
				refs_seen += cnt;
				if (refs_seen > n_refs) { // cells sharing a run: the tables are not the builder's; refuse rather than overflow
							return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_scene_create: cells/mapping_table runs overlap");
				}
				entries[c * rmd::kEntrySlots] = rmd::CellEntry{(uint32_t)ids.size(), cnt};
				ids.insert(ids.end(), g.mapping_table + off + 1, g.mapping_table + off + 1 + cnt);
			}
			const int64_t sx = (int64_t)g.resolution[0], sxz = (int64_t)g.resolution[0] * (int64_t)g.resolution[2]; // Q5: res.z where res.y is meant
			const int64_t delta[7] = {0, 1, -1, sx, -sx, sxz, -sxz};
			std::vector<uint32_t> fresh;
			std::vector<uint64_t> listed_by((size_t)g.n_tris, ~0ull); // triangle -> the (cell, slot) pass that last saw it in a predecessor's list
			for (uint64_t c = 0; c < g.n_cells; c++) {
				const rmd::CellEntry full = entries[c * rmd::kEntrySlots];
				const uint32_t *mine = g.mapping_table + g.cells[c] + 1;
				for (uint32_t s = 1; s < rmd::kEntrySlots; s++) {
					rmd::CellEntry &e = entries[c * rmd::kEntrySlots + s];
					e = full;
					if (s == 7u || full.count == 0u) continue;
					const int64_t prev = (int64_t)c - delta[s];
					if (prev < 0 || prev >= (int64_t)g.n_cells || prev == (int64_t)c) continue; // no such predecessor: never asked for
					const uint32_t poff = g.cells[prev], pcnt = g.mapping_table[poff];
					if (pcnt == 0u) continue;
					const uint32_t *theirs = g.mapping_table + poff + 1;
					fresh.clear();
					const uint64_t pass = c * rmd::kEntrySlots + s;
					for (uint32_t j = 0; j < pcnt; j++) listed_by[theirs[j]] = pass;
					for (uint32_t k = 0; k < full.count; k++)
						if (listed_by[mine[k]] != pass) fresh.push_back(mine[k]);
					if (fresh.size() == full.count) continue; // nothing to leave out: shares the full list
					e = rmd::CellEntry{(uint32_t)ids.size(), (uint32_t)fresh.size()};
					ids.insert(ids.end(), fresh.begin(), fresh.end());
					if (ids.size() > 0xFFFFFFFFull) {
									return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "rmd_scene_create: triangle index lists exceed 2^32 entries");
					}
				}
			}
		}
		out.aux.assign((size_t)g.n_tris * 4, 0.0);
		for (uint64_t ti = 0; ti < g.n_tris; ti++) rmd::triangle_aux(g.tri_pos + (size_t)ti * 9, out.aux.data() + (size_t)ti * 4);
		out.spheres.assign((size_t)g.n_tris * 4, 0.0);
		out.sphere_kb = 0.0;
		for (uint64_t ti = 0; ti < g.n_tris; ti++) {
			double kb = 0.0;
			rmd::triangle_sphere(g.tri_pos + (size_t)ti * 9, out.spheres.data() + (size_t)ti * 4, kb);
			out.sphere_kb = std::max(out.sphere_kb, kb);
		}
	}
	return RMD_OK;
}

// What rmd_scene_create derives from the caller's objects on the host, before anything is uploaded: the device records, whether the scene's
// parameters are regular, the pairs of opposite planes, the axis rule's walls and the object loops' turns.  A function of its own because the
// host-only probe rmd_probe_primary_candidates (probe.cpp) needs exactly what a scene would hold, without a device.
extern "C++" rmd_status rmd::derive_scene_objects(rmd_context *ctx, const rmd_object *objects, uint32_t n_objects, uint32_t n_grids, int64_t axis_pairs_tunable, rmd::SceneObjects &out) {
	std::vector<rmd::DevObject> &hobj = out.objs;
	hobj.assign(n_objects, rmd::DevObject{});
	bool regular = true;
	for (uint32_t i = 0; i < n_objects; i++) {
		const rmd_object &o = objects[i];
		rmd::DevObject &d = hobj[i];
		std::memset(&d, 0, sizeof(d));
		if (o.geometry_kind > RMD_GEOM_GRID) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_scene_create: unknown geometry kind");
		if (o.material.kind > RMD_MAT_EMISSION) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_scene_create: unknown material kind");
		if (o.geometry_kind == RMD_GEOM_GRID && o.grid_index >= n_grids) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_scene_create: grid_index out of range");
		d.geometry_kind = o.geometry_kind, d.grid_index = o.grid_index, d.material_kind = o.material.kind;
		for (int a = 0; a < 3; a++) d.origin[a] = o.origin[a], d.normal[a] = o.normal[a], d.color[a] = o.material.color[a];
		d.radius = o.radius;
		// the GGX angle roughness^2 * sqrt(u / (1 - u)) must stay inside sincos_cw's reduction range (device_core.hpp)
		if (o.material.kind != RMD_MAT_EMISSION && std::fabs(o.material.roughness) > rmd::kMaxRoughness)
			return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "rmd_scene_create: |roughness| > 512 is not supported");
		// (the bounce weight is formed as ONE quotient whose denominator holds (roughness^2 / 8)^2 for a surface seen from behind: it must not underflow)
		if (o.material.kind != RMD_MAT_EMISSION && o.material.roughness != 0.0 && std::fabs(o.material.roughness) < rmd::kMinRoughness)
			return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "rmd_scene_create: 0 < |roughness| < 1e-12 is not supported");
		d.roughness = o.material.roughness;
		d.metalness = o.material.kind == RMD_MAT_METAL ? 1.0 : 0.0; // src/trace.rs:248-249
		// Is this object inside the class of parameters for which "a path whose throughput is exactly (0, 0, 0) contributes exactly (0, 0, 0)" is
		// proved?  The proof needs every later vertex of such a path to have a FINITE radiance (0 x NaN = NaN, src/trace.rs:
		// 281-282, :315-318).  Outside the class — an Emission of (inf, 0, 0), a NaN or infinite colour / position / normal, coordinates so large that a
		// hit point overflows, a sphere of radius 0 (normalize(P - centre) of a hit at the centre), a material of roughness 0 (geometry_schlick_ggx is
		// 0 / 0 for a surface seen from behind, :372-378) — the reference's sample can be NaN without any mesh, so flags 0 traces such a scene's
		// black paths on, as it does a scene with a grid (make_params).
		{
			auto tame = [](double v) { return std::fabs(v) <= 1e150; }; // finite, and no sum or product of two of them overflows
			bool ok = true;
			if (o.geometry_kind != RMD_GEOM_GRID)
				for (int a = 0; a < 3; a++) ok = ok && tame(o.origin[a]);
			if (o.geometry_kind == RMD_GEOM_PLANE)
				for (int a = 0; a < 3; a++) ok = ok && tame(o.normal[a]);
			if (o.geometry_kind == RMD_GEOM_SPHERE) ok = ok && tame(o.radius) && o.radius != 0.0 && o.radius * o.radius > 0.0;
			for (int a = 0; a < 3; a++) ok = ok && tame(o.material.color[a]);
			if (o.material.kind != RMD_MAT_EMISSION) ok = ok && tame(o.material.roughness) && o.material.roughness != 0.0;
			regular = regular && ok;
		}
		if (o.material.kind == RMD_MAT_DIFFUSE && o.material.color[0] == 0.0 && o.material.color[1] == 0.0 && o.material.color[2] == 0.0) d.flags |= rmd::kObjBlackDiffuse;
	}
	// pair_opposite_planes: plane j is tested together with the first earlier, still unpaired plane i whose normal is its exact negation
	// (device_core.hpp: plane_pair_intersect — the facing conditions of such planes exclude each other, one division serves both)
	for (uint32_t j = 0; j < n_objects; j++) {
		if (hobj[j].geometry_kind != RMD_GEOM_PLANE) continue;
		for (uint32_t i = 0; i < j; i++) {
			if (hobj[i].geometry_kind != RMD_GEOM_PLANE || hobj[i].pair_info != 0u) continue;
			bool opposite = true; // NaN components compare unequal: never paired
			for (int a = 0; a < 3; a++) opposite = opposite && hobj[j].normal[a] == -hobj[i].normal[a];
			if (!opposite) continue;
			hobj[i].pair_info = rmd::kPairTestedAtPartner | j, hobj[j].pair_info = i + 1u;
			break;
		}
	}
	// ... and a pair whose normals are exactly +e_k and -e_k — the walls of an axis-aligned room — is tested with one component of the ray instead of
	// three dot products (scene_split.hpp: axis_pairs_visit has the argument for "same bits"): one pair per axis, in scenes of regular parameters
	uint32_t axis_pairs = 0;
	for (uint32_t j = 0; j < n_objects && j < 1023u && regular && axis_pairs_tunable != 1; j++) {
		if (hobj[j].geometry_kind != RMD_GEOM_PLANE || hobj[j].pair_info == 0u || (hobj[j].pair_info & rmd::kPairTestedAtPartner)) continue;
		const uint32_t i = hobj[j].pair_info - 1u;
		int k = -1, nonzero = 0;
		for (int a = 0; a < 3; a++)
			if (hobj[i].normal[a] != 0.0) nonzero++, k = a;
		if (nonzero != 1 || (hobj[i].normal[k] != 1.0 && hobj[i].normal[k] != -1.0) || ((axis_pairs >> (10 * k)) & 1023u) != 0u) continue;
		axis_pairs |= (j + 1u) << (10 * k);
		hobj[j].flags |= rmd::kObjAxisPair | ((uint32_t)k << rmd::kObjAxisShift) | (hobj[i].normal[k] == 1.0 ? rmd::kObjAxisEarlierIsPlus : 0u);
		hobj[i].flags |= rmd::kObjAxisPair;
		hobj[j].partner_origin_k = hobj[i].origin[k];
		hobj[j].pair_info = rmd::kPairTestedAtPartner | rmd::kPairAxis | i; // the object loops pass both planes by ("tested at its partner's turn"):
		hobj[i].pair_info |= rmd::kPairAxis;                                 // their turn is axis_pairs_visit's, ahead of the loop
	}
	// the axis pairs as the axis rule reads them (device_types.hpp: AxisWalls)
	{
		rmd::AxisWalls *walls = out.walls;
		std::memset(walls, 0, 3 * sizeof(rmd::AxisWalls));
		for (int k = 0; k < 3; k++) {
			const uint32_t f = (axis_pairs >> (10 * k)) & 1023u;
			if (f == 0u) continue;
			const uint32_t j = f - 1u, i = hobj[j].pair_info & 0x3FFFFFFFu; // the later and the earlier plane of the pair
			const bool e_plus = (hobj[j].flags & rmd::kObjAxisEarlierIsPlus) != 0u;
			walls[k].o_plus = e_plus ? hobj[i].origin[k] : hobj[j].origin[k], walls[k].o_minus = e_plus ? hobj[j].origin[k] : hobj[i].origin[k];
			walls[k].idx_plus = e_plus ? i : j, walls[k].idx_minus = e_plus ? j : i;
		}
	}
	// the object loops' turns (device_types.hpp: RenderParams::visit_mask): a plane tested at its partner's turn or by the axis rule has none
	out.visit_mask = 0ull, out.grid_mask = 0ull;
	for (uint32_t i = 0; i < n_objects && i < 64u; i++) {
		if (!(hobj[i].geometry_kind == RMD_GEOM_PLANE && (hobj[i].pair_info & rmd::kPairTestedAtPartner))) out.visit_mask |= 1ull << i;
		if (hobj[i].geometry_kind == RMD_GEOM_GRID) out.grid_mask |= 1ull << i;
	}
	out.regular = regular, out.axis_pairs = axis_pairs;
	return RMD_OK;
}

static rmd_status scene_create_impl(rmd_context *ctx, const rmd_object *objects, uint32_t n_objects, const rmd_grid_desc *grids, uint32_t n_grids,
                                    rmd_scene **out) {
	if (rmd_status s = bind(ctx)) return s;
	if (!out || (n_objects && !objects) || (n_grids && !grids)) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_scene_create: null argument");
	rmd::SceneObjects derived;
	if (rmd_status s = rmd::derive_scene_objects(ctx, objects, n_objects, n_grids, ctx->tunable[RMD_TUNE_AXIS_PAIRS], derived)) return s;
	std::vector<rmd::DevObject> &hobj = derived.objs;
	const bool regular = derived.regular;
	const uint32_t axis_pairs = derived.axis_pairs;
	// (the scene under construction: an early return or an exception — std::bad_alloc from one of the host-side tables: a 256^3 grid needs a
	// gigabyte for its cell entries alone — releases what has been uploaded)
	auto sc = std::make_unique<rmd_scene>();
	sc->ctx = ctx, sc->n_objects = n_objects, sc->n_grids = n_grids, sc->regular = regular;
	sc->axis_pairs = axis_pairs;
	// the axis pairs as the axis rule reads them, behind the table's last record (device_types.hpp: AxisWalls)
	rmd::DevObject walls_block;
	std::memset(&walls_block, 0, sizeof(walls_block));
	std::memcpy(&walls_block, derived.walls, sizeof(derived.walls));
	sc->visit_mask = derived.visit_mask, sc->grid_mask = derived.grid_mask;
	for (uint32_t i = 0; i < n_objects; i++)
		if (objects[i].geometry_kind == RMD_GEOM_PLANE) sc->planes.insert(sc->planes.end(), objects[i].origin, objects[i].origin + 3), sc->planes.insert(sc->planes.end(), objects[i].normal, objects[i].normal + 3);
	// the generation trips' own candidate sets and the items' tile classes (primary_candidates.hpp): a regular scene without a grid, unless
	// RMD_TUNE_AXIS_PAIRS says 1 or 2 (neither) or 3 (no tile classes)
	sc->primary_cull = rmd::primary_cull_bits(regular, n_grids, ctx->tunable[RMD_TUNE_AXIS_PAIRS]);
	for (uint32_t i = 0; i < n_objects; i++) sc->n_grid_objects += objects[i].geometry_kind == RMD_GEOM_GRID ? 1u : 0u;
	auto upload = [&](const void *src, size_t bytes, void **dst) -> hipError_t {
		*dst = nullptr;
		rmd::DeviceBuffer b;
		hipError_t e = b.alloc(bytes ? bytes : 16);
		if (e != hipSuccess) return e;
		*dst = b.as<void>();
		sc->owned.push_back(std::move(b));
		if (bytes) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
		return e;
	};
	std::vector<rmd::DevGrid> hgrid(n_grids);
	for (uint32_t gi = 0; gi < n_grids; gi++) {
		const rmd_grid_desc &g = grids[gi];
		rmd::DevGrid &d = hgrid[gi];
		std::memset(&d, 0, sizeof(d));
		// the derived tables: from the rmd_grid_build this description came from (derived once, kept there), or made here
		std::shared_ptr<const GridDerived> derived;
		{
			rmd_grid_build *gb = const_cast<rmd_grid_build *>(g.built);
			const bool from_build = gb && gb->cells.data() == g.cells && gb->cells.size() == g.n_cells && gb->mapping.data() == g.mapping_table &&
			                        gb->mapping.size() == g.n_mapping && gb->pos.data() == g.tri_pos && gb->nrm.data() == g.tri_nrm && gb->pos.size() == g.n_tris * 9;
			std::unique_lock<std::mutex> lock;
			if (from_build) {
				lock = std::unique_lock<std::mutex>(gb->derived_mutex);
				derived = std::static_pointer_cast<const GridDerived>(gb->derived);
			}
			if (!derived) {
				auto fresh = std::make_shared<GridDerived>();
				if (rmd_status st = derive_grid_tables(ctx, g, *fresh)) return st;
				derived = fresh;
				if (from_build) gb->derived = fresh;
			}
		}
		const std::vector<unsigned char> &recs = derived->recs;
		const std::vector<rmd::CellEntry> &entries = derived->entries;
		const std::vector<uint32_t> &ids = derived->ids;
		const std::vector<double> &aux = derived->aux;
		for (int a = 0; a < 3; a++) {
			d.bbox_min[a] = g.bbox_min[a], d.bbox_max[a] = g.bbox_max[a], d.cell_size[a] = g.cell_size[a];
			d.inv_cell_size[a] = rmd::exact_reciprocal(g.cell_size[a]);
			d.res[a] = g.resolution[a];
			if (a == 2) sc->walk_steps_bound = std::max<uint32_t>(sc->walk_steps_bound, (uint32_t)std::min<uint64_t>((uint64_t)g.resolution[0] + g.resolution[1] + g.resolution[2] + 3u, 0xFFFFFFFFull));
		}
		d.n_cells = g.n_cells, d.n_tris = g.n_tris;
		uint64_t last_nonempty = 0;
		bool any_nonempty = false;
		for (uint64_t c = 0; c < g.n_cells; c++)
			if (entries[c * rmd::kEntrySlots].count) last_nonempty = c, any_nonempty = true;
		// occupancy bitmask for LDS: bit i covers cells [i << shift, (i+1) << shift); only up to the last non-empty cell
		// the mask covers every cell of the array when that fits the budget (the stepping loop's lean form then needs no clamp of the index),
		// else the cells up to the last non-empty one (indices past it read the all-zero word that ends every mask)
		uint64_t covered = any_nonempty ? last_nonempty + 1 : 0;
		size_t budget_bytes = rmd::kMaskBudgetBytes;
		if (ctx->tunable[RMD_TUNE_MASK_BUDGET] > 0) budget_bytes = (size_t)ctx->tunable[RMD_TUNE_MASK_BUDGET]; // forces coarser masks
		if (budget_bytes < 64) budget_bytes = 64;
		if (budget_bytes > rmd::kMaskBudgetBytes) budget_bytes = rmd::kMaskBudgetBytes;
		const size_t budget_words = budget_bytes / 4 / n_grids;
		if (budget_words < 2) // one data word + the all-zero pad word is the smallest mask
			return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "rmd_scene_create: too many grids for the LDS occupancy-mask budget");
		if ((g.n_cells + 31) / 32 + 1 <= budget_words) covered = g.n_cells;
		uint32_t shift = 0;
		while (shift < 63 && ((covered >> shift) + 31) / 32 + 1 > budget_words) shift++;
		const uint64_t bits = covered ? ((covered - 1) >> shift) + 1 : 0;
		std::vector<uint32_t> mask((size_t)((bits + 31) / 32) + 1, 0u); // + one all-zero word: indices past the mask read it
		for (uint64_t c = 0; c < covered; c++)
			if (entries[c * rmd::kEntrySlots].count) mask[(c >> shift) >> 5] |= 1u << ((c >> shift) & 31u);
		d.mask_bits = (uint32_t)bits, d.mask_shift = shift, d.mask_n_words = (uint32_t)mask.size();
		d.mask_lds_word = sc->mask_words_total;
		sc->mask_words_total += (uint32_t)((mask.size() + 3) & ~(size_t)3);
		void *p = nullptr;
		RMD_HIP(ctx, upload(entries.data(), entries.size() * sizeof(rmd::CellEntry), &p));
		d.cell_entries = (const rmd::CellEntry *)p;
		RMD_HIP(ctx, upload(ids.data(), ids.size() * sizeof(uint32_t), &p));
		d.tri_ids = (const uint32_t *)p;
		RMD_HIP(ctx, upload(recs.data(), recs.size(), &p));
		d.tri_recs = p;
		RMD_HIP(ctx, upload(mask.data(), mask.size() * sizeof(uint32_t), &p));
		d.mask_words = (const uint32_t *)p;
		RMD_HIP(ctx, upload(g.tri_pos, g.n_tris * 9 * sizeof(double), &p));
		d.tri_pos = (const double *)p;
		RMD_HIP(ctx, upload(g.tri_nrm, g.n_tris * 9 * sizeof(double), &p));
		d.tri_nrm = (const double *)p;
		RMD_HIP(ctx, upload(aux.data(), aux.size() * sizeof(double), &p));
		d.tri_aux = (const double *)p;
		RMD_HIP(ctx, upload(derived->spheres.data(), derived->spheres.size() * sizeof(double), &p));
		d.tri_sph = (const double *)p, d.sph_kb = derived->sphere_kb;
	}
	void *p = nullptr;
	hobj.push_back(walls_block); // (uploaded behind the table; n_objects does not count it)
	RMD_HIP(ctx, upload(hobj.data(), hobj.size() * sizeof(rmd::DevObject), &p));
	sc->d_objects = (rmd::DevObject *)p;
	RMD_HIP(ctx, upload(hgrid.data(), hgrid.size() * sizeof(rmd::DevGrid), &p));
	sc->d_grids = (rmd::DevGrid *)p;
	*out = sc.release();
	return RMD_OK;
}

rmd_status rmd_scene_create(rmd_context *ctx, const rmd_object *objects, uint32_t n_objects, const rmd_grid_desc *grids, uint32_t n_grids,
                            rmd_scene **out) {
	if (out) *out = nullptr;
	return rmd::guarded(ctx, "rmd_scene_create", [&] { return scene_create_impl(ctx, objects, n_objects, grids, n_grids, out); });
}

// (the launches that read the scene's tables are waited for in the body; `owned` is freed after it)
rmd_scene::~rmd_scene() {
	if (ctx) {
		(void)hipSetDevice(ctx->device);
		(void)hipStreamSynchronize(ctx->stream);
	}
}

void rmd_scene_destroy(rmd_scene *scene) { delete scene; }

rmd_status rmd_framebuffer_alloc(rmd_context *ctx, uint32_t width, uint32_t height, double **out_dev) {
	if (rmd_status s = bind(ctx)) return s;
	if (!out_dev || width == 0 || height == 0) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_framebuffer_alloc: bad argument");
	size_t bytes = (size_t)width * height * 3 * sizeof(double);
	RMD_HIP(ctx, hipMalloc((void **)out_dev, bytes));
	RMD_HIP(ctx, hipMemsetAsync(*out_dev, 0, bytes, ctx->stream));
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return RMD_OK;
}
rmd_status rmd_framebuffer_free(rmd_context *ctx, double *dev) {
	if (rmd_status s = bind(ctx)) return s;
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	RMD_HIP(ctx, hipFree(dev));
	return RMD_OK;
}
rmd_status rmd_framebuffer_zero(rmd_context *ctx, double *dev, size_t n) {
	if (rmd_status s = bind(ctx)) return s;
	if (!dev) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_framebuffer_zero: null pointer");
	RMD_HIP(ctx, hipMemsetAsync(dev, 0, n * sizeof(double), ctx->stream));
	return RMD_OK;
}
rmd_status rmd_framebuffer_download(rmd_context *ctx, const double *dev, double *host, size_t n) {
	if (rmd_status s = bind(ctx)) return s;
	if (!dev || !host) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_framebuffer_download: null pointer");
	RMD_HIP(ctx, hipMemcpyAsync(host, dev, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return rmd::check_fault(ctx); // a frame cut short by a device fault is not handed out as a result
}
rmd_status rmd_framebuffer_upload(rmd_context *ctx, const double *host, double *dev, size_t n) {
	if (rmd_status s = bind(ctx)) return s;
	if (!dev || !host) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_framebuffer_upload: null pointer");
	RMD_HIP(ctx, hipMemcpyAsync(dev, host, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return RMD_OK;
}

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
	// Samples per pass of a split launch: the scratch buffer holds n_wave_tiles x 64 x samples x 32 bytes (the whole C3 frame at 500 spp
	// is 33 GB, one launch).  By default it may take an eighth of the device memory that is free right now (RMD_TUNE_SCRATCH_CAP_MB
	// overrides), never less than 8 samples per pass; what does not fit runs as several passes.  The device may still refuse the
	// allocation — other contexts, ranks or tenants hold memory, or the cap was set beyond it: the pass is then halved until a buffer
	// can be had (the old one stays until a larger one exists), and when not even 8 samples fit the launch runs unsplit (one wave per
	// wave tile, no scratch).  Every route gives the same frame bit for bit.
	uint32_t per_pass = P.sample_count;
	if (buffered) {
		const size_t bytes_per_sample = (size_t)P.n_work * 64u * rmd::kSampleStride * sizeof(double);
		size_t cap;
		if (ctx->tunable[RMD_TUNE_SCRATCH_CAP_MB] > 0) cap = (size_t)ctx->tunable[RMD_TUNE_SCRATCH_CAP_MB] << 20;
		else {
			size_t free_b = 0, total_b = 0;
			RMD_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
			cap = (free_b + ctx->sample_buf.bytes()) / 8; // the buffer this context already holds counts as available to it
		}
		if (bytes_per_sample * per_pass > cap) per_pass = (uint32_t)(cap / bytes_per_sample);
		// (the mesh kernel numbers a pass's 32-byte sectors in 32 bits: render_kernel.hpp, PathId)
		const uint64_t sectors_per_sample = (uint64_t)P.n_work * 64u;
		if (sectors_per_sample * per_pass > 0xFFFFFFFFull) per_pass = (uint32_t)(0xFFFFFFFFull / sectors_per_sample);
		if (per_pass < 8u) per_pass = 8u;
		if (per_pass > P.sample_count) per_pass = P.sample_count;
		// (a frame of more than 2^32 / 8 / 64 = 8.4 M wave tiles — 537 Mpixel — cannot number even the smallest pass's sectors in 32 bits: unsplit, no scratch)
		if (sectors_per_sample * per_pass > 0xFFFFFFFFull) split = 1u, buffered = false, per_pass = P.sample_count;
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
				split = 1u, buffered = false, per_pass = P.sample_count;
				break;
			}
			per_pass = per_pass / 2u < 8u ? 8u : per_pass / 2u;
		}
	}
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
		// Persistent split launches of scenes with grids keep their paths in queues in device memory (render_kernel.hpp: render_wave_queued;
		// RMD_TUNE_PATH_QUEUES: 1 = never): kQueuePaths entries on each of a resident wave's two stacks, 192 bytes a path — 49 KB a wave, 200 MB
		// for the 4,096 resident waves of an MI355X — allocated at the first launch that wants them.  A device that cannot provide them runs
		// the lane-per-path form (render_wave): the same frame bit for bit.
		if (persistent_pass && buffered && scene->n_grids != 0u && ctx->tunable[RMD_TUNE_PATH_QUEUES] != 1) {
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
		}
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
	if (P.debug_flags & 24u) {
		unsigned long long h[64];
		RMD_HIP(ctx, hipMemcpyAsync(h, ctx->debug_counters.as<void>(), sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
		RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
		if ((P.debug_flags & 16u) && ctx->last_launch.queued) {
			static const char *kinds[3] = {"GEN  ", "SHADE", "WALK "};
			for (int k = 0; k < 3; k++)
				std::fprintf(stderr, "[rmd queued stamps, cycles] %s trips=%llu fetch=%llu make_ray=%llu simple=%llu walk=%llu ray_push=%llu classify=%llu stores=%llu\n", kinds[k], h[k * 8 + 7],
				             h[k * 8 + 0], h[k * 8 + 1], h[k * 8 + 2], h[k * 8 + 3], h[k * 8 + 4], h[k * 8 + 5], h[k * 8 + 6]);
			std::fprintf(stderr, "[rmd queued stamps, cycles] inside the walks: init=%llu stepping=%llu entry_wait=%llu scan=%llu (chunk search+load+test)=%llu hits=%llu tail=%llu\n",
			             h[24], h[25], h[26], h[27], h[29], h[30], h[31]);
		} else if (P.debug_flags & 16u)
			std::fprintf(stderr, "[rmd stamps, cycles] wave_total=%llu next_ray=%llu simple=%llu walk=%llu classify=%llu | walk: init=%llu stepping=%llu entry_wait=%llu scan=%llu (chunk search+load+test)=%llu hits=%llu tail=%llu\n",
			             h[0], h[1], h[2], h[3], h[4], h[8], h[9], h[10], h[11], h[13], h[14], h[15]);
		else
			std::fprintf(stderr, "[rmd debug] walk_calls=%llu walkers=%llu calls_with_walkers=%llu rounds=%llu wave_steps=%llu lane_steps=%llu test_rounds=%llu tests=%llu chunks=%llu | main_iterations=%llu live_lanes=%llu lanes_with_ray=%llu | stepping iterations with <= 4 / 8 / 16 lanes: %llu / %llu / %llu, with <= 8 lanes while tests wait: %llu\n",
			             h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[8], h[9], h[10], h[11], h[12], h[7], h[13], h[14], h[15]);
		if ((P.debug_flags & 16u) == 0u)
			std::fprintf(stderr, "[rmd debug] sphere pre-test: pairs passed=%llu full chunks=%llu | pairs dropped that pass the reference's test (flag 64; must be 0)=%llu\n", h[17], h[18], h[16]);
		if ((P.debug_flags & 16u) == 0u && (P.debug_flags & 512u))
			std::fprintf(stderr, "[rmd debug] primary candidates: lanes checked=%llu sphere turns left out=%llu trips with two axis pairs left out=%llu | cleared spheres that register a hit (must be 0)=%llu closest hits that differ from the full visit's (must be 0)=%llu\n",
			             h[32], h[35], h[36], h[33], h[34]);
		if ((P.debug_flags & 16u) == 0u && ctx->last_launch.buffered && scene->n_grids == 0u) // (the role-sorted spheres kernel: render_wave_sorted)
			std::fprintf(stderr, "[rmd debug] lobe trips: diffuse trips=%llu diffuse hits shaded=%llu ggx trips=%llu ggx hits shaded=%llu | hits parked: diffuse=%llu ggx=%llu\n", h[37], h[38], h[39],
			             h[40], h[41], h[42]);
		if ((P.debug_flags & 16u) == 0u && ctx->last_launch.buffered && scene->n_grids == 0u) // (its items' tile classes: primary_candidates.hpp)
			std::fprintf(stderr, "[rmd debug] tile classes: general items=%llu emitter items=%llu black items=%llu | black rounds=%llu cut short=%llu samples ended in pass A=%llu survivors=%llu | samples checked against their full path=%llu that are not what the class says (must be 0)=%llu rays that hit another object than the wall (must be 0)=%llu\n",
			             h[48], h[49], h[50], h[52], h[54], h[51], h[53], h[55], h[56], h[57]);
		if ((P.debug_flags & 16u) == 0u && ctx->last_launch.queued)
			std::fprintf(stderr, "[rmd debug] path queues: rays pushed=%llu (of them walks put aside=%llu) rays held in their lanes=%llu hits pushed=%llu hits held in their lanes=%llu\n", h[19], h[22], h[23], h[20], h[21]);
	}
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

static rmd_status tile_error_impl(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height,
                                  uint32_t sample_count, double floor, const rmd_tile_rect *rects, uint32_t n_rects, double *out_err_host) {
	if (rmd_status s = bind(ctx)) return s;
	for (uint32_t i = 0; i < n_rects; i++)
		if ((uint64_t)rects[i].left + rects[i].width > width || (uint64_t)rects[i].top + rects[i].height > height)
			return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_tile_error: tile rectangle outside the framebuffer");
	rmd::DeviceBuffer d; // the device scratch (it outlives the wait below)
	if (n_rects != 0) {
		// device buffer: [rects: 16 bytes each][errors: 8 bytes each]
		const size_t rect_bytes = (size_t)n_rects * sizeof(rmd_tile_rect);
		RMD_HIP(ctx, d.alloc(rect_bytes + (size_t)n_rects * sizeof(double)));
		rmd_tile_rect *d_rects = d.as<rmd_tile_rect>();
		double *d_err = reinterpret_cast<double *>(d.as<unsigned char>() + rect_bytes);
		RMD_HIP(ctx, hipMemcpyAsync(d_rects, rects, rect_bytes, hipMemcpyHostToDevice, ctx->stream));
		RMD_HIP(ctx, rmd::launch_tile_error(ctx->stream, accum_dev, accum_sq_dev, d_rects, n_rects, width, sample_count, floor, d_err));
		RMD_HIP(ctx, hipMemcpyAsync(out_err_host, d_err, (size_t)n_rects * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	}
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return rmd::check_fault(ctx); // the sums came from launches this call has waited for
}

rmd_status rmd_tile_error(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height, uint32_t sample_count,
                          double floor, const rmd_tile_rect *rects, uint32_t n_rects, double *out_err_host) {
	if (!accum_dev || !accum_sq_dev || width == 0 || height == 0 || (n_rects && (!rects || !out_err_host)))
		return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_tile_error: bad argument");
	if (accum_sq_dev == accum_dev) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_tile_error: accum_sq_dev must not alias accum_dev");
	if (!(floor > 0.0) || !std::isfinite(floor)) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_tile_error: floor must be finite and > 0");
	return rmd::guarded(ctx, "rmd_tile_error", [&] {
		return tile_error_impl(ctx, accum_dev, accum_sq_dev, width, height, sample_count, floor, rects, n_rects, out_err_host);
	});
}

// ---------------------------------------------------------------- first-hit feature buffers (features.hip)
rmd_status rmd_feature_buffer_alloc(rmd_context *ctx, uint32_t width, uint32_t height, double **out_dev) {
	if (rmd_status s = bind(ctx)) return s;
	if (!out_dev || width == 0 || height == 0) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_feature_buffer_alloc: bad argument");
	const size_t bytes = (size_t)width * height * RMD_FEATURE_CHANNELS * sizeof(double);
	RMD_HIP(ctx, hipMalloc((void **)out_dev, bytes));
	RMD_HIP(ctx, hipMemsetAsync(*out_dev, 0, bytes, ctx->stream));
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return RMD_OK;
}

static rmd_status render_features_impl(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                                       const rmd_tile_rect *tiles, uint32_t n_tiles, double *feat_dev, double *feat_sq_dev) {
	rmd_settings st = *settings;
	st.bounce_limit = 1u; // ignored: the pass traces the first segment only
	{
		const char *why = nullptr;
		if (!rmd::denoise_rects_ok(tiles, n_tiles, camera->backbuffer_width, camera->backbuffer_height, &why))
			return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, std::string("rmd_render_features: ") + why);
	}
	if (rmd_status s = bind(ctx)) return s;
	if (rmd_status s = check_render_args(ctx, scene, camera, &st)) return s;
	if (rmd_status s = prepare_wave_tiles(ctx, camera, tiles, n_tiles)) return s;
	rmd::RenderParams P = rmd::make_params(ctx, scene, camera, &st);
	P.n_work = ctx->n_wave_tiles;
	// (neither the context's events nor its launch record are touched: rmd_last_kernel_ms / rmd_last_launch_info keep describing the last render)
	RMD_HIP(ctx, rmd::launch_features(ctx->stream, P, scene->d_objects, scene->d_grids, ctx->wave_tiles.as<rmd::WaveTile>(), feat_dev, feat_sq_dev));
	return RMD_OK;
}

rmd_status rmd_render_features_async(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                                     const rmd_tile_rect *tiles, uint32_t n_tiles, double *feat_dev, double *feat_sq_dev) {
	if (!scene || !camera || !settings) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_render_features: null scene/camera/settings");
	if (!feat_dev || (n_tiles && !tiles)) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_render_features: null tiles/feat pointer");
	if (feat_sq_dev != nullptr) { // the two W*H*7-double ranges must not overlap
		const unsigned __int128 bytes = (unsigned __int128)camera->backbuffer_width * camera->backbuffer_height * RMD_FEATURE_CHANNELS * sizeof(double);
		const unsigned __int128 f = (uintptr_t)feat_dev, g = (uintptr_t)feat_sq_dev;
		if (f < g + bytes && g < f + bytes) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_render_features: feat_sq_dev must not alias feat_dev");
	}
	return rmd::guarded(ctx, "rmd_render_features", [&] { return render_features_impl(ctx, scene, camera, settings, tiles, n_tiles, feat_dev, feat_sq_dev); });
}

rmd_status rmd_render_features(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                               const rmd_tile_rect *tiles, uint32_t n_tiles, double *feat_dev, double *feat_sq_dev) {
	if (rmd_status s = rmd_render_features_async(ctx, scene, camera, settings, tiles, n_tiles, feat_dev, feat_sq_dev)) return s;
	return rmd_context_synchronize(ctx);
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

// ---------------------------------------------------------------- tile rectangles <-> packed host buffers
namespace {
// Checks the rects, builds the table {rect, first pixel} and makes slot `sl`'s device buffers large enough.  Returns the packed pixel count.
rmd_status prepare_transfer(rmd_context *ctx, rmd_context::TransferSlot &sl, uint32_t W, uint32_t H, const rmd_tile_rect *rects, uint32_t n_rects, uint64_t &n_pixels) {
	n_pixels = 0;
	sl.h_table.resize((size_t)n_rects * (sizeof(rmd_tile_rect) + sizeof(uint64_t)));
	rmd_tile_rect *hr = reinterpret_cast<rmd_tile_rect *>(sl.h_table.data());
	uint64_t *hf = reinterpret_cast<uint64_t *>(sl.h_table.data() + (size_t)n_rects * sizeof(rmd_tile_rect));
	for (uint32_t i = 0; i < n_rects; i++) {
		const rmd_tile_rect &r = rects[i];
		if ((uint64_t)r.left + r.width > W || (uint64_t)r.top + r.height > H)
			return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "tile transfer: tile rectangle outside the framebuffer");
		hr[i] = r, hf[i] = n_pixels;
		n_pixels += (uint64_t)r.width * r.height;
	}
	RMD_HIP(ctx, sl.packed.grow((size_t)n_pixels * 3 * sizeof(double)));
	RMD_HIP(ctx, sl.table.grow(sl.h_table.size()));
	if (!sl.packed_ready) RMD_HIP(ctx, hipEventCreateWithFlags(&sl.packed_ready, hipEventDisableTiming));
	if (!sl.copied) RMD_HIP(ctx, hipEventCreateWithFlags(&sl.copied, hipEventDisableTiming));
	if (!ctx->copy_stream) RMD_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
	return RMD_OK;
}
rmd_status wait_slot(rmd_context *ctx, rmd_context::TransferSlot &sl) {
	if (sl.in_flight) {
		RMD_HIP(ctx, hipEventSynchronize(sl.copied));
		sl.in_flight = false;
	}
	return RMD_OK;
}
} // namespace

static rmd_status download_tiles_async_impl(rmd_context *ctx, const double *dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                                            uint32_t n_rects, double *host_packed) {
	if (rmd_status s = bind(ctx)) return s;
	if (!dev || !host_packed || (n_rects && !rects) || width == 0 || height == 0) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_framebuffer_download_tiles: bad argument");
	if (n_rects == 0) return RMD_OK;
	rmd_context::TransferSlot &sl = ctx->transfer[ctx->next_transfer];
	ctx->next_transfer ^= 1u;
	if (rmd_status s = wait_slot(ctx, sl)) return s; // a third download waits for the first
	uint64_t n_pixels = 0;
	if (rmd_status s = prepare_transfer(ctx, sl, width, height, rects, n_rects, n_pixels)) return s;
	const rmd_tile_rect *d_rects = sl.table.as<rmd_tile_rect>();
	const uint64_t *d_first = reinterpret_cast<const uint64_t *>(sl.table.as<unsigned char>() + (size_t)n_rects * sizeof(rmd_tile_rect));
	// main stream: table, pack (behind the renders enqueued before); copy stream: the download (renders enqueued after this overlap it)
	RMD_HIP(ctx, hipMemcpyAsync(sl.table.as<void>(), sl.h_table.data(), sl.h_table.size(), hipMemcpyHostToDevice, ctx->stream));
	RMD_HIP(ctx, rmd::launch_tile_copy(ctx->stream, true, const_cast<double *>(dev), sl.packed.as<double>(), d_rects, d_first, n_rects, width));
	RMD_HIP(ctx, hipEventRecord(sl.packed_ready, ctx->stream));
	RMD_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, sl.packed_ready, 0));
	RMD_HIP(ctx, hipMemcpyAsync(host_packed, sl.packed.as<double>(), (size_t)n_pixels * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->copy_stream));
	RMD_HIP(ctx, hipEventRecord(sl.copied, ctx->copy_stream));
	sl.in_flight = true;
	return RMD_OK;
}

rmd_status rmd_framebuffer_download_tiles_async(rmd_context *ctx, const double *dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                                                uint32_t n_rects, double *host_packed) {
	return rmd::guarded(ctx, "rmd_framebuffer_download_tiles", [&] { return download_tiles_async_impl(ctx, dev, width, height, rects, n_rects, host_packed); });
}

rmd_status rmd_context_wait_transfers(rmd_context *ctx) {
	if (rmd_status s = bind(ctx)) return s;
	for (auto &sl : ctx->transfer)
		if (rmd_status s = wait_slot(ctx, sl)) return s;
	return rmd::check_fault(ctx); // the tiles came from launches that have completed by now
}

rmd_status rmd_framebuffer_download_tiles(rmd_context *ctx, const double *dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                                          uint32_t n_rects, double *host_packed) {
	if (rmd_status s = rmd_framebuffer_download_tiles_async(ctx, dev, width, height, rects, n_rects, host_packed)) return s;
	return rmd_context_wait_transfers(ctx);
}

static rmd_status upload_tiles_impl(rmd_context *ctx, const double *host_packed, double *dev, uint32_t width, uint32_t height,
                                    const rmd_tile_rect *rects, uint32_t n_rects) {
	if (rmd_status s = bind(ctx)) return s;
	if (!dev || !host_packed || (n_rects && !rects) || width == 0 || height == 0) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_framebuffer_upload_tiles: bad argument");
	if (n_rects == 0) return RMD_OK;
	rmd_context::TransferSlot &sl = ctx->transfer[ctx->next_transfer];
	ctx->next_transfer ^= 1u;
	if (rmd_status s = wait_slot(ctx, sl)) return s;
	uint64_t n_pixels = 0;
	if (rmd_status s = prepare_transfer(ctx, sl, width, height, rects, n_rects, n_pixels)) return s;
	const rmd_tile_rect *d_rects = sl.table.as<rmd_tile_rect>();
	const uint64_t *d_first = reinterpret_cast<const uint64_t *>(sl.table.as<unsigned char>() + (size_t)n_rects * sizeof(rmd_tile_rect));
	RMD_HIP(ctx, hipMemcpyAsync(sl.table.as<void>(), sl.h_table.data(), sl.h_table.size(), hipMemcpyHostToDevice, ctx->stream));
	RMD_HIP(ctx, hipMemcpyAsync(sl.packed.as<double>(), host_packed, (size_t)n_pixels * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	RMD_HIP(ctx, rmd::launch_tile_copy(ctx->stream, false, dev, sl.packed.as<double>(), d_rects, d_first, n_rects, width));
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the caller's buffer and the table are free again
	return rmd::check_fault(ctx); // (this wait has also waited for every render enqueued before it)
}
rmd_status rmd_framebuffer_upload_tiles(rmd_context *ctx, const double *host_packed, double *dev, uint32_t width, uint32_t height,
                                        const rmd_tile_rect *rects, uint32_t n_rects) {
	return rmd::guarded(ctx, "rmd_framebuffer_upload_tiles", [&] { return upload_tiles_impl(ctx, host_packed, dev, width, height, rects, n_rects); });
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

static rmd_status resolve_tonemap_impl(rmd_context *ctx, const double *accum_dev, uint32_t width, uint32_t height, uint32_t sample_count,
                                       double exposure, double gamma, uint8_t *out_rgb8_host) {
	if (rmd_status s = bind(ctx)) return s;
	if (!accum_dev || !out_rgb8_host || width == 0 || height == 0 || sample_count == 0)
		return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_resolve_tonemap: bad argument");
	const size_t n_pixels = (size_t)width * height;
	if (n_pixels > 0xFFFFFFFFull) return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "rmd_resolve_tonemap: more than 2^32-1 pixels");
	// device buffer: [rgb8: 3 n bytes, padded to 4][count: 1 word][flagged pixel indices: n words]
	const size_t rgb_bytes = (n_pixels * 3 + 3) & ~(size_t)3;
	rmd::DeviceBuffer scratch;
	RMD_HIP(ctx, scratch.alloc(rgb_bytes + 4 + n_pixels * 4));
	uint8_t *d = scratch.as<uint8_t>();
	uint32_t *d_count = reinterpret_cast<uint32_t *>(d + rgb_bytes), *d_list = d_count + 1;
	const double sc = (double)sample_count, inv_gamma = 1.0 / gamma;
	uint32_t n_flagged = 0;
	std::vector<uint32_t> list;
	std::vector<double> px;
	hipError_t e = hipMemsetAsync(d_count, 0, 4, ctx->stream);
	if (e == hipSuccess) e = rmd::launch_tonemap(ctx->stream, accum_dev, d, n_pixels, sc, exposure, inv_gamma, d_list, d_count);
	if (e == hipSuccess) e = hipMemcpyAsync(out_rgb8_host, d, n_pixels * 3, hipMemcpyDeviceToHost, ctx->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(&n_flagged, d_count, 4, hipMemcpyDeviceToHost, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	if (e == hipSuccess && n_flagged != 0) {
		// the pixels whose byte an ulp of exp / pow could decide: recomputed with the host libm, as the reference does every pixel
		list.resize(n_flagged);
		e = hipMemcpy(list.data(), d_list, (size_t)n_flagged * 4, hipMemcpyDeviceToHost);
		const bool whole = n_flagged > 1024u; // many (a synthetic frame): one download of the frame instead of a copy per pixel
		if (e == hipSuccess && whole) {
			px.resize(n_pixels * 3);
			e = hipMemcpy(px.data(), accum_dev, n_pixels * 3 * sizeof(double), hipMemcpyDeviceToHost);
		}
		for (uint32_t k = 0; k < n_flagged && e == hipSuccess; k++) {
			const size_t i = list[k];
			double a[3];
			if (whole) a[0] = px[i * 3], a[1] = px[i * 3 + 1], a[2] = px[i * 3 + 2];
			else e = hipMemcpy(a, accum_dev + i * 3, sizeof(a), hipMemcpyDeviceToHost);
			if (e != hipSuccess) break;
			double v[3];
			bool ok = true;
			for (int c = 0; c < 3; c++) {
				const double p = a[c] / sc; // src/trace.rs:95
				double tm = 1.0 - std::exp(p * -1.0 * exposure); // cli_old/src/main.rs:165
				tm = std::pow(tm, inv_gamma);                    // :166
				v[c] = tm * 255.0;
				ok = ok && (v[c] > -1.0 && v[c] < 256.0); // :176 cast::<u8>()
			}
			for (int c = 0; c < 3; c++) out_rgb8_host[i * 3 + c] = ok ? (uint8_t)v[c] : (uint8_t)0;
		}
	}
	RMD_HIP(ctx, e);
	// the frame came from launches this call has waited for: one that was cut short by a device fault is not handed out as an image
	return rmd::check_fault(ctx);
}
rmd_status rmd_resolve_tonemap(rmd_context *ctx, const double *accum_dev, uint32_t width, uint32_t height, uint32_t sample_count,
                               double exposure, double gamma, uint8_t *out_rgb8_host) {
	return rmd::guarded(ctx, "rmd_resolve_tonemap", [&] { return resolve_tonemap_impl(ctx, accum_dev, width, height, sample_count, exposure, gamma, out_rgb8_host); });
}

// The same stage over tile rectangles, each at its own sample count, into rmd_framebuffer_download_tiles's layout (resolve_tiles.hip; the table and
// the way back from a flagged packed pixel: resolve_tiles_host.hpp).  Scratch on the context: [rgb8: 3 P bytes, padded to 16][flag count: 16 bytes]
// [flagged packed pixels: P words, padded to 16][runs].
static rmd_status resolve_tonemap_tiles_impl(rmd_context *ctx, const double *accum_dev, const double *accum2_dev, uint32_t width, uint32_t height,
                                             const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects, double exposure, double gamma,
                                             uint8_t *out) {
	const char *name = "rmd_resolve_tonemap_tiles: ";
	if (rmd_status s = bind(ctx)) return s;
	if (!accum_dev || width == 0 || height == 0 || (n_rects && (!rects || !rect_sample_counts)))
		return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, std::string(name) + "bad argument");
	const size_t frame_doubles = (size_t)width * height * 3;
	const uintptr_t lo1 = reinterpret_cast<uintptr_t>(accum_dev), lo2 = reinterpret_cast<uintptr_t>(accum2_dev), frame_bytes = frame_doubles * sizeof(double);
	if (accum2_dev && lo2 < lo1 + frame_bytes && lo1 < lo2 + frame_bytes)
		return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, std::string(name) + "accum2_dev overlaps accum_dev");
	std::vector<uint64_t> first;
	if (!rmd::resolve_first_pixels(rects, n_rects, width, height, first))
		return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, std::string(name) + "tile rectangle outside the framebuffer");
	const uint64_t n_pixels = first[n_rects];
	if (n_pixels > 0xFFFFFFFFull) return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, std::string(name) + "more than 2^32-1 packed pixels");
	if (n_pixels == 0) return RMD_OK;
	if (!out) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, std::string(name) + "null output for rects that hold pixels");
	const std::vector<rmd::ResolveRun> runs = rmd::resolve_runs(rects, rect_sample_counts, n_rects, first);
	if (runs.size() > 0x7FFFFFFFull) return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, std::string(name) + "more than 2^31-1 workgroups");
	const size_t rgb_bytes = ((size_t)n_pixels * 3 + 15) & ~(size_t)15, list_bytes = ((size_t)n_pixels * 4 + 15) & ~(size_t)15;
	const size_t table_bytes = runs.size() * sizeof(rmd::ResolveRun);
	// The stream is waited for before anything is enqueued (the call waits for the frame's renders in any case): the table's upload and the downloads
	// below, which may go to pageable memory, are then made on an idle stream, as rmd_resolve_tonemap's are by every caller here
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	RMD_HIP(ctx, ctx->resolve_tiles_scratch.grow(rgb_bytes + 16 + list_bytes + table_bytes));
	ctx->resolve_tiles_table.assign(reinterpret_cast<const unsigned char *>(runs.data()), reinterpret_cast<const unsigned char *>(runs.data()) + table_bytes);
	uint8_t *d = ctx->resolve_tiles_scratch.as<uint8_t>();
	uint32_t *d_count = reinterpret_cast<uint32_t *>(d + rgb_bytes), *d_list = reinterpret_cast<uint32_t *>(d + rgb_bytes + 16);
	rmd::ResolveRun *d_runs = reinterpret_cast<rmd::ResolveRun *>(d + rgb_bytes + 16 + list_bytes);
	const double inv_gamma = 1.0 / gamma;
	uint32_t n_flagged = 0;
	std::vector<uint32_t> list;
	std::vector<double> px, px2;
	hipError_t e = hipMemsetAsync(d_count, 0, 4, ctx->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(d_runs, ctx->resolve_tiles_table.data(), table_bytes, hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess)
		e = rmd::launch_resolve_tiles(ctx->stream, accum_dev, accum2_dev, width, d_runs, (uint32_t)runs.size(), exposure, inv_gamma, d, d_list, d_count);
	if (e == hipSuccess) e = hipMemcpyAsync(out, d, (size_t)n_pixels * 3, hipMemcpyDeviceToHost, ctx->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(&n_flagged, d_count, 4, hipMemcpyDeviceToHost, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	if (e == hipSuccess && n_flagged != 0) {
		// as rmd_resolve_tonemap: the pixels whose byte an ulp of exp / pow could decide, recomputed with the host libm
		list.resize(n_flagged);
		e = hipMemcpy(list.data(), d_list, (size_t)n_flagged * 4, hipMemcpyDeviceToHost);
		const bool whole = n_flagged > 1024u; // many: one download of the sums instead of a copy per pixel
		if (e == hipSuccess && whole) {
			px.resize(frame_doubles);
			e = hipMemcpy(px.data(), accum_dev, frame_doubles * sizeof(double), hipMemcpyDeviceToHost);
			if (e == hipSuccess && accum2_dev) {
				px2.resize(frame_doubles);
				e = hipMemcpy(px2.data(), accum2_dev, frame_doubles * sizeof(double), hipMemcpyDeviceToHost);
			}
		}
		for (uint32_t k = 0; k < n_flagged && e == hipSuccess; k++) {
			const uint64_t q = list[k];
			const rmd::ResolvePixel at = rmd::resolve_locate(rects, n_rects, first, q);
			const size_t i = ((size_t)at.x + (size_t)at.y * width) * 3;
			double a[3], b[3] = {0.0, 0.0, 0.0};
			if (whole) {
				for (int c = 0; c < 3; c++) a[c] = px[i + c];
				if (accum2_dev)
					for (int c = 0; c < 3; c++) b[c] = px2[i + c];
			} else {
				e = hipMemcpy(a, accum_dev + i, sizeof(a), hipMemcpyDeviceToHost);
				if (e == hipSuccess && accum2_dev) e = hipMemcpy(b, accum2_dev + i, sizeof(b), hipMemcpyDeviceToHost);
			}
			if (e != hipSuccess) break;
			const double sc = (double)rect_sample_counts[at.rect];
			double v[3];
			bool ok = true;
			for (int c = 0; c < 3; c++) {
				const double s = accum2_dev ? a[c] + b[c] : a[c];
				const double p = s / sc; // src/trace.rs:95
				double tm = 1.0 - std::exp(p * -1.0 * exposure); // cli_old/src/main.rs:165
				tm = std::pow(tm, inv_gamma);                    // :166
				v[c] = tm * 255.0;
				ok = ok && (v[c] > -1.0 && v[c] < 256.0); // :176 cast::<u8>()
			}
			for (int c = 0; c < 3; c++) out[q * 3 + c] = ok ? (uint8_t)v[c] : (uint8_t)0;
		}
	}
	RMD_HIP(ctx, e);
	return rmd::check_fault(ctx);
}
rmd_status rmd_resolve_tonemap_tiles(rmd_context *ctx, const double *accum_dev, const double *accum2_dev, uint32_t width, uint32_t height,
                                     const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects, double exposure, double gamma,
                                     uint8_t *out_rgb8_host_packed) {
	return rmd::guarded(ctx, "rmd_resolve_tonemap_tiles", [&] {
		return resolve_tonemap_tiles_impl(ctx, accum_dev, accum2_dev, width, height, rects, rect_sample_counts, n_rects, exposure, gamma, out_rgb8_host_packed);
	});
}

// The luminance histogram of the same rects (luma_histogram.hip; luma_bins.hpp: the luminance and the counter of a pixel).  The argument rules are
// rmd_resolve_tonemap_tiles's, in its order, and all of them come before the context is looked at.  Scratch on the context: [261 counters, padded to
// 16 bytes][runs].
static_assert(sizeof(rmd_luma_histogram) == (rmd::kLumaCounters + 1) * sizeof(uint64_t) && RMD_LUMA_BINS == rmd::kLumaBins, "luma_bins.hpp mirrors include/raymond_hip.h");
static_assert(offsetof(rmd_luma_histogram, below) == rmd::kLumaBelow * 8 && offsetof(rmd_luma_histogram, above) == rmd::kLumaAbove * 8 &&
              offsetof(rmd_luma_histogram, zero) == rmd::kLumaZero * 8 && offsetof(rmd_luma_histogram, negative) == rmd::kLumaNegative * 8 &&
              offsetof(rmd_luma_histogram, not_finite) == rmd::kLumaNotFinite * 8 && offsetof(rmd_luma_histogram, pixels) == rmd::kLumaCounters * 8,
              "the device's counters are the struct's fields in order");
static rmd_status luminance_histogram_tiles_impl(rmd_context *ctx, const double *accum_dev, const double *accum2_dev, uint32_t width, uint32_t height,
                                                 const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects, rmd_luma_histogram *out) {
	const char *name = "rmd_luminance_histogram_tiles: ";
	if (!accum_dev || width == 0 || height == 0 || (n_rects && (!rects || !rect_sample_counts)))
		return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, std::string(name) + "bad argument");
	const size_t frame_doubles = (size_t)width * height * 3;
	const uintptr_t lo1 = reinterpret_cast<uintptr_t>(accum_dev), lo2 = reinterpret_cast<uintptr_t>(accum2_dev), frame_bytes = frame_doubles * sizeof(double);
	if (accum2_dev && lo2 < lo1 + frame_bytes && lo1 < lo2 + frame_bytes)
		return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, std::string(name) + "accum2_dev overlaps accum_dev");
	std::vector<uint64_t> first;
	if (!rmd::resolve_first_pixels(rects, n_rects, width, height, first))
		return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, std::string(name) + "tile rectangle outside the framebuffer");
	const uint64_t n_pixels = first[n_rects];
	if (n_pixels > 0xFFFFFFFFull) return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, std::string(name) + "more than 2^32-1 packed pixels");
	if (!out) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, std::string(name) + "null out_host");
	if (rmd_status s = bind(ctx)) return s;
	std::memset(out, 0, sizeof(*out));
	if (n_pixels == 0) return RMD_OK;
	const std::vector<rmd::ResolveRun> runs = rmd::resolve_runs(rects, rect_sample_counts, n_rects, first);
	if (runs.size() > 0x7FFFFFFFull) return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, std::string(name) + "more than 2^31-1 workgroups");
	const size_t counter_bytes = ((size_t)rmd::kLumaCounters * sizeof(uint64_t) + 15) & ~(size_t)15, table_bytes = runs.size() * sizeof(rmd::ResolveRun);
	// as rmd_resolve_tonemap_tiles: the stream is waited for first, so that the table's upload and the counters' download are made on an idle stream
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	RMD_HIP(ctx, ctx->luma_scratch.grow(counter_bytes + table_bytes));
	ctx->luma_table.assign(reinterpret_cast<const unsigned char *>(runs.data()), reinterpret_cast<const unsigned char *>(runs.data()) + table_bytes);
	uint8_t *d = ctx->luma_scratch.as<uint8_t>();
	uint64_t *d_counters = reinterpret_cast<uint64_t *>(d);
	rmd::ResolveRun *d_runs = reinterpret_cast<rmd::ResolveRun *>(d + counter_bytes);
	uint64_t counters[rmd::kLumaCounters];
	hipError_t e = hipMemsetAsync(d_counters, 0, counter_bytes, ctx->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(d_runs, ctx->luma_table.data(), table_bytes, hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess) e = rmd::launch_luma_histogram(ctx->stream, accum_dev, accum2_dev, width, d_runs, (uint32_t)runs.size(), d_counters);
	if (e == hipSuccess) e = hipMemcpyAsync(counters, d_counters, sizeof(counters), hipMemcpyDeviceToHost, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	RMD_HIP(ctx, e);
	std::memcpy(out, counters, sizeof(counters)); // (the fields in order: the static_asserts above)
	for (uint32_t i = 0; i < rmd::kLumaCounters; i++) out->pixels += counters[i];
	return rmd::check_fault(ctx);
}
rmd_status rmd_luminance_histogram_tiles(rmd_context *ctx, const double *accum_dev, const double *accum2_dev, uint32_t width, uint32_t height,
                                         const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects, rmd_luma_histogram *out_host) {
	return rmd::guarded(ctx, "rmd_luminance_histogram_tiles", [&] {
		return luminance_histogram_tiles_impl(ctx, accum_dev, accum2_dev, width, height, rects, rect_sample_counts, n_rects, out_host);
	});
}

// The exposure that puts a percentile of a histogram's luminance at `target` before gamma: host arithmetic only, no context, no device.
rmd_status rmd_exposure_from_histogram(const rmd_luma_histogram *h, double percentile, double target, double *out_exposure) {
	return rmd::guarded(nullptr, "rmd_exposure_from_histogram", [&]() -> rmd_status {
		const char *name = "rmd_exposure_from_histogram: ";
		if (!h || !out_exposure) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, std::string(name) + "null pointer");
		if (!(percentile > 0.0 && percentile <= 1.0)) // (a NaN fails both)
			return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, std::string(name) + "percentile must be finite and in (0, 1]");
		if (!(target > 0.0 && target < 1.0)) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, std::string(name) + "target must be finite and in (0, 1)");
		uint64_t n = h->below + h->above;
		for (uint32_t i = 0; i < RMD_LUMA_BINS; i++) n += h->bins[i];
		if (n == 0) {
			*out_exposure = 1.0;
			return RMD_OK;
		}
		const double want = std::ceil(percentile * (double)n);
		uint64_t rank = want >= 18446744073709551616.0 ? n : (uint64_t)want; // (2^64: (double)n may have rounded up to it)
		rank = std::min(std::max<uint64_t>(rank, 1), n);
		double y = 0x1p-32; // the walk stops in `below`
		uint64_t seen = h->below;
		if (seen < rank) {
			y = 0x1p32; // ... or in `above`, when no bin reaches the rank
			for (uint32_t i = 0; i < RMD_LUMA_BINS; i++) {
				seen += h->bins[i];
				if (seen >= rank) {
					y = std::ldexp(1.0 + (double)(i % 4u + 1u) * 0.25, (int)(i / 4u) + rmd::kLumaMinExponent); // the bin's upper edge
					break;
				}
			}
		}
		*out_exposure = -std::log1p(-target) / y;
		return RMD_OK;
	});
}

// The squared slope of the library's tone curve per luminance counter, for rmd_tile_weighted_error: host arithmetic only, no context, no device.
rmd_status rmd_display_weights(double exposure, double gamma, double display_floor, double *out_weights) {
	return rmd::guarded(nullptr, "rmd_display_weights", [&]() -> rmd_status {
		const char *name = "rmd_display_weights: ";
		if (!out_weights) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, std::string(name) + "null pointer");
		if (!(exposure > 0.0) || !std::isfinite(exposure)) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, std::string(name) + "exposure must be finite and > 0");
		if (!(gamma > 0.0) || !std::isfinite(gamma)) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, std::string(name) + "gamma must be finite and > 0");
		if (!(display_floor > 0.0 && display_floor < 1.0)) // (a NaN fails both)
			return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, std::string(name) + "display_floor must be finite and in (0, 1)");
		const double inv_g = 1.0 / gamma;
		const double y_floor = -std::log1p(-std::pow(display_floor, gamma)) / exposure;
		auto weight = [&](double y) {
			const double t = -std::expm1(-y * exposure);
			const double slope = inv_g * std::pow(t, inv_g - 1.0) * exposure * std::exp(-y * exposure);
			const double w = slope * slope;
			if (!(w == w)) return 0.0;                                      // inf * 0: a factor has vanished
			return w > 1.7976931348623157e308 ? 1.7976931348623157e308 : w; // overflow: the largest finite double
		};
		// the bin's centre, exact: 2^E (1 + (M + 0.5) / 4); luminances under the one that displays at display_floor take that luminance's slope
		for (uint32_t i = 0; i < RMD_LUMA_BINS; i++)
			out_weights[i] = weight(std::max(std::ldexp(1.0 + ((double)(i % 4u) + 0.5) * 0.25, (int)(i / 4u) + rmd::kLumaMinExponent), y_floor));
		out_weights[rmd::kLumaBelow] = out_weights[rmd::kLumaZero] = out_weights[rmd::kLumaNegative] = weight(y_floor);
		out_weights[rmd::kLumaAbove] = weight(0x1p32);
		return RMD_OK;
	});
}

} // extern "C"
