// Library-internal declarations shared by api.cpp, api_scene.cpp, api_frame.cpp, api_denoise.cpp, probe.cpp, comm.cpp, grid_build.cpp and grid_build_gpu.hip.
#pragma once
#include <stdint.h>

#include <cmath>
#include <limits>
#include <algorithm>
#include <cstring>

#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/raymond_hip.h"

#ifdef RMD_WITH_HIP
#include <hip/hip_runtime_api.h>

#include "device_types.hpp"
#include "primary_candidates.hpp"
#include "work_list.hpp"

// The one mapping of a failed HIP call to a status: returns from the calling function with the call's text and HIP's own.
#define RMD_HIP(ctx, call)                                                                                      \
	do {                                                                                                        \
		hipError_t e_ = (call);                                                                                 \
		if (e_ != hipSuccess) return rmd::fail(ctx, e_ == hipErrorOutOfMemory ? RMD_ERR_OUT_OF_MEMORY : RMD_ERR_HIP, \
		                                       std::string(#call) + ": " + hipGetErrorString(e_));              \
	} while (0)

namespace rmd {
// Device memory the library holds: one hipMalloc block and its size in bytes, freed when its owner goes — a context, a scene, or the frame of
// an entry point whichever way it leaves.  Pointers handed to the caller (rmd_framebuffer_alloc, rmd_feature_buffer_alloc) stay raw.
class DeviceBuffer {
public:
	DeviceBuffer() = default;
	DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
	// (what `o` held replaces this buffer's block only once it exists: the allocate-first order of the sample scratch, api.cpp)
	DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
		if (this != &o) (void)release(), p_ = o.p_, bytes_ = o.bytes_, o.p_ = nullptr, o.bytes_ = 0;
		return *this;
	}
	~DeviceBuffer() { (void)release(); }
	hipError_t release() {
		const hipError_t e = p_ ? hipFree(p_) : hipSuccess;
		p_ = nullptr, bytes_ = 0;
		return e;
	}
	// Free first, then allocate: after a refused allocation the buffer is empty and its size 0, so the next call tries again.
	hipError_t alloc(size_t bytes) {
		hipError_t e = release();
		if (e == hipSuccess) e = hipMalloc(&p_, bytes);
		if (e == hipSuccess) bytes_ = bytes;
		else p_ = nullptr;
		return e;
	}
	hipError_t grow(size_t bytes) { return bytes <= bytes_ ? hipSuccess : alloc(bytes); }
	size_t bytes() const { return bytes_; }
	template <class T>
	T *as() const { return static_cast<T *>(p_); }

private:
	void *p_ = nullptr;
	size_t bytes_ = 0;
};
} // namespace rmd

struct rmd_context {
	int device = 0;
	hipStream_t stream = nullptr;
	bool owns_stream = false;
	hipEvent_t ev_start = nullptr, ev_stop = nullptr;
	bool timed = false;
	std::string last_error;
	// cached wave-tile table (device) for the rect list of the previous call
	std::vector<rmd_tile_rect> cached_rects;
	uint32_t cached_W = 0, cached_H = 0;
	rmd::DeviceBuffer wave_tiles; // rmd::WaveTile
	uint32_t n_wave_tiles = 0;
	rmd::DeviceBuffer sample_buf; // per-sample radiance scratch of split launches (api.cpp: choose_split)
	uint32_t wave_slots = 0; // CUs x waves per CU the render kernels can keep resident
	uint32_t n_cus = 0;
	rmd::DeviceBuffer work_counter;   // next work item of a persistent launch (render_kernel.hpp)
	rmd::DeviceBuffer queue_buf;      // the resident waves' path queues (render_kernel.hpp: render_wave_queued), allocated at the first launch that uses them
	rmd::DeviceBuffer tile_done;      // split launches: finished waves per wave tile, a uint32 each (render_kernel.hpp)
	rmd::DeviceBuffer debug_counters; // walk diagnostics (DIAG builds, RMD_DEBUG=8|16)
	rmd::DeviceBuffer atrous_region_scratch; // rmd_denoise_atrous_dual_region's planes, count images and tables (api_denoise.cpp): grown when a call needs more, kept between calls
	size_t atrous_region_slope_offset = 0, atrous_region_slope_pixels = 0; // the last sloped region call's slope planes in that block and its W*H (0: none yet), for rmd_probe_atrous_region_slope_planes
	// A run-table call's block, [head][runs] (api_frame.cpp: upload_run_table), grown when a call needs more and kept between calls, and the table's host copy, alive until
	// its upload has completed.  The head: rmd_resolve_tonemap_tiles's packed bytes, flag count and flag list; rmd_luminance_histogram_tiles's 261 counters
	struct RunTable {
		rmd::DeviceBuffer block;
		std::vector<unsigned char> host;
	} resolve_tiles, luma;
	rmd::DeviceBuffer despike_scratch; // rmd_despike's count image, rect-index image, rects, counts and per-rect spike counters (api_denoise.cpp): grown when a call needs more, kept between calls
	rmd::DeviceBuffer despike_dual_scratch; // rmd_despike_dual's two count images, rect-index image, rects, both counts and per-rect spike counters (api_denoise.cpp): grown when a call needs more, kept between calls
	rmd::DeviceBuffer tile_luma_scratch; // rmd_tile_luma_error's rects, counts and per-rect results (api_denoise.cpp): grown when a call needs more, kept between calls
	rmd::DeviceBuffer tile_weighted_scratch; // rmd_tile_weighted_error's rects, counts, weights and per-rect results (api_denoise.cpp): grown when a call needs more, kept between calls
	rmd::DeviceBuffer tile_weighted_dual_scratch; // rmd_tile_weighted_error_dual's rects, weights and per-rect results (api_denoise.cpp): grown when a call needs more, kept between calls
	rmd::DeviceBuffer ids_matte_scratch; // rmd_ids_matte's counter of pixels with other != 0 and its sorted distinct keys (api.cpp): grown when a call needs more, kept between calls
	rmd::DeviceBuffer ao_resolve_scratch; // rmd_ao_resolve's counter of pixels without a first hit, 16 bytes (api.cpp): allocated by the first call, kept between calls
	// fault words (device_types.hpp: kFault*): pinned host memory mapped into the device's address space.  A wave whose loop runs past its bound
	// writes here; the host looks after every wait for the stream (api.cpp: check_fault) — a plain host load, no copy
	uint32_t *h_fault = nullptr, *d_fault = nullptr;
	// tile transfers (rmd_framebuffer_{download,upload}_tiles, api_frame.cpp): two staging slots — packed pixels, rect table, prefix table on the device — so that a
	// second download can be packed while the first is still being copied; the copy stream; per slot the event its copy ends with
	struct TransferSlot {
		rmd::DeviceBuffer packed; // doubles
		rmd::DeviceBuffer table;  // n_rects x (rmd_tile_rect, uint64 first)
		hipEvent_t packed_ready = nullptr, copied = nullptr;
		bool in_flight = false;
		std::vector<unsigned char> h_table; // the host copy of the table stays alive until its upload has completed
	} transfer[2];
	uint32_t next_transfer = 0;
	hipStream_t copy_stream = nullptr;
	// Tunables (include/raymond_hip.h: rmd_context_set_tunable).  Defaults come from the environment, read ONCE when the
	// context is created; none of them changes a result.
	int64_t tunable[RMD_TUNE_COUNT] = {};
	uint32_t debug_flags = 0; // RMD_DEBUG, honoured by DIAG builds only
	uint32_t tail_x2 = rmd::kTailTilesPerSlotX2, tail_parts = rmd::kTailParts; // the spheres kernel's work list (api.cpp: plan_work_list); only a sweep build changes them
	rmd_launch_info last_launch = {}; // rmd_last_launch_info
	// Waits for both streams, then destroys them, the events and the fault words; the buffers above are freed after that (api.cpp).
	~rmd_context();
};

struct rmd_scene {
	rmd_context *ctx = nullptr;
	uint32_t n_objects = 0, n_grids = 0;
	uint32_t n_grid_objects = 0; // objects whose geometry is a grid
	uint32_t mask_words_total = 0; // LDS words of the grids' occupancy masks
	uint32_t axis_pairs = 0; // RenderParams::axis_pairs
	unsigned long long visit_mask = ~0ull, grid_mask = ~0ull; // RenderParams::visit_mask / grid_mask
	uint32_t walk_steps_bound = 0; // RenderParams::walk_steps_bound
	uint32_t primary_cull = 0; // the scene's half of RenderParams::primary_cull: regular, no grid; by RMD_TUNE_AXIS_PAIRS when it was created 3 (candidate
	                           // sets and tile classes: 0), 1 (candidate sets only: 3) or 0 (neither: 1, 2)
	bool regular = true; // every parameter the kernel reads is finite and inside the class for which ending zero-throughput paths is exact (api_scene.cpp: derive_scene_objects)
	std::vector<double> planes; // origin and normal of every plane object, six numbers each: make_params asks whether the camera lies ON one
	rmd::DevObject *d_objects = nullptr;
	rmd::DevGrid *d_grids = nullptr;
	std::vector<rmd::DeviceBuffer> owned; // every device allocation of this scene
	~rmd_scene(); // waits for the context's stream before they are freed (api_scene.cpp)
};
#endif

// Result of a grid build (host or GPU): owns the arrays a rmd_grid_desc points at.
struct rmd_grid_build {
	double bbox_min[3], bbox_max[3], cell_size[3];
	uint32_t res[3];
	std::vector<uint32_t> cells, mapping;
	std::vector<double> pos, nrm;
	// what rmd_scene_create derives from these arrays (api_scene.cpp: GridDerived), kept for the next upload of the same grid
	std::shared_ptr<void> derived;
	std::mutex derived_mutex;
};

namespace rmd {
// Mesh::find_mesh_bounds (mesh.rs:123-140) for both grid builders: the fold over all vertices in order, from the reference's seeds (Q9).  The
// reference folds with f64::min / f64::max and leaves the sign of a zero bound — a tie of +0.0 and -0.0 — to the platform; std::fmin leaves it to
// the compiler (g++ calls glibc, where the second operand wins; clang expands it inline, and which zero survives depends on how it orders the
// operands — in the builders' loop the first).  The project's rule is the oracle's: the LATER vertex wins the tie, a NaN coordinate is skipped.
// Written as comparisons so that every compiler gives the same bytes.
inline void mesh_bounds(const double *tri_pos, uint64_t n_tris, double bbox_min[3], double bbox_max[3]) {
	static const double seed_min[3] = {125125.0, 1251251.0, 12512512.0}, seed_max[3] = {-123125.0, -125123.0, -512123.0};
	for (int a = 0; a < 3; a++) bbox_min[a] = seed_min[a], bbox_max[a] = seed_max[a];
	for (uint64_t i = 0; i < n_tris * 3; i++)
		for (int a = 0; a < 3; a++) {
			const double v = tri_pos[i * 3 + a];
			if (v <= bbox_min[a]) bbox_min[a] = v;
			if (v >= bbox_max[a]) bbox_max[a] = v;
		}
}
// Per-triangle constants of the Heron normal (triangle.rs:47-68): the two sides and the area that do not depend on the
// hit point, with exactly the operations of device_core.hpp (dist = sqrt(((dx*dx + dy*dy) + dz*dz)), heron_area_of_sides):
// every operation is a correctly rounded IEEE one and this file is compiled with -ffp-contract=off, so the values are
// bit-identical to what the kernel would compute.  out = { |p0p1|, |p0p2|, area(p0,p1,p2), exact_reciprocal(area) }.
// r = 1.0 / b for use by the device's div_by(a, b, r) (device_core.hpp), or NaN when that shortcut is not exact for this
// divisor: Markstein's correction needs the correctly rounded reciprocal (this division) and fails for a divisor whose
// significand is all ones; zero, non-finite and extreme divisors are left to the IEEE division as well.
inline double exact_reciprocal(double b) {
	uint64_t bits;
	std::memcpy(&bits, &b, 8);
	const double m = std::fabs(b);
	if (!(m >= 0x1p-500 && m <= 0x1p500) || (bits & 0xFFFFFFFFFFFFFull) == 0xFFFFFFFFFFFFFull) return std::nan("");
	return 1.0 / b;
}
// A sphere around a triangle for the walk's pre-test (grid_walk.hpp): a (ray, triangle) pair whose LINE passes the centre at more than
//     sqrt(r2a + kb * |centre - origin|^2)
// cannot pass triangle.rs:11-44 and is not tested.  What has to hold is that the reference's test, AS COMPUTED in binary64, fails for every pair
// the pre-test drops.  In exact arithmetic the test accepts lines through the triangle, all of which pass within r of the centre of any sphere
// that contains the three vertices.  As computed, the barycentric coordinates carry an error of at most ~4 eps |s| |h| / |a| with |a| >= 1e-8
// (EPSILON), |h| <= L (longest edge) and |s| <= |centre - origin| + L: a point up to 4.4e-8 L^2 (|d| + L) outside the triangle can still be
// accepted.  Both terms are taken a hundredfold: the radius grows by 4.4e-6 L^3 (and 1e-3 of itself, and an ulp-sized absolute term), the
// allowance k |d| with k = 4.4e-6 L^2 enters through (r + k|d|)^2 <= 1.01 r^2 + 101 k^2 |d|^2, and 32 eps |d|^2 covers the cancellation in
// |d|^2 - (d.rd)^2 of the pre-test itself.  The sphere is the smallest one around the vertices (the longest edge's, or the circumscribed one).
inline void triangle_sphere(const double *p9, double out[4], double &kb) {
	const double *P[3] = {p9, p9 + 3, p9 + 6};
	auto sub = [](const double *a, const double *b, double *o) { for (int i = 0; i < 3; i++) o[i] = a[i] - b[i]; };
	auto dot = [](const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
	auto cross = [](const double *a, const double *b, double *o) { o[0] = a[1] * b[2] - a[2] * b[1], o[1] = a[2] * b[0] - a[0] * b[2], o[2] = a[0] * b[1] - a[1] * b[0]; };
	double e[3][3], l2[3];
	sub(P[2], P[1], e[0]), sub(P[0], P[2], e[1]), sub(P[1], P[0], e[2]); // edge i is opposite vertex i
	for (int i = 0; i < 3; i++) l2[i] = dot(e[i], e[i]);
	const int longest = l2[0] >= l2[1] && l2[0] >= l2[2] ? 0 : (l2[1] >= l2[2] ? 1 : 2);
	const double L = std::sqrt(l2[longest]);
	double c[3];
	for (int i = 0; i < 3; i++) c[i] = 0.5 * (P[(longest + 1) % 3][i] + P[(longest + 2) % 3][i]);
	double dv[3];
	sub(P[longest], c, dv);
	if (dot(dv, dv) > 0.25 * l2[longest]) { // acute: the circumscribed sphere's centre, A + (|b|^2 (a x b) x a + |a|^2 b x (a x b)) / (2 |a x b|^2)
		double a[3], b[3], n[3], t1[3], t2[3];
		sub(P[1], P[0], a), sub(P[2], P[0], b), cross(a, b, n);
		const double n2 = dot(n, n);
		cross(n, a, t1), cross(b, n, t2);
		if (n2 > 0.0 && std::isfinite(n2))
			for (int i = 0; i < 3; i++) c[i] = P[0][i] + (dot(b, b) * t1[i] + dot(a, a) * t2[i]) / (2.0 * n2);
	}
	double r2 = 0.0;
	for (int v = 0; v < 3; v++) { // whatever the centre came out as: the radius that contains the vertices
		sub(P[v], c, dv);
		r2 = std::max(r2, dot(dv, dv));
	}
	const double cmax = std::max(std::fabs(c[0]), std::max(std::fabs(c[1]), std::fabs(c[2])));
	const double r = std::sqrt(r2) * 1.001 + 4.4e-6 * L * L * L + 1e-12 * (1.0 + cmax);
	out[0] = c[0], out[1] = c[1], out[2] = c[2], out[3] = 1.01 * r * r;
	const double k = 4.4e-6 * L * L;
	kb = 101.0 * k * k + 32.0 * 2.220446049250313e-16;
	if (!(std::isfinite(out[0]) && std::isfinite(out[1]) && std::isfinite(out[2]) && std::isfinite(out[3]) && std::isfinite(kb)))
		out[0] = out[1] = out[2] = 0.0, out[3] = std::numeric_limits<double>::infinity(), kb = 0.0; // a triangle with non-finite vertices: never dropped
}
inline void triangle_aux(const double *p9, double out[4]) {
	auto dist = [](const double *a, const double *b) {
		const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
		return std::sqrt((dx * dx + dy * dy) + dz * dz);
	};
	const double ab = dist(p9, p9 + 3), ac = dist(p9, p9 + 6), bc = dist(p9 + 3, p9 + 6);
	const double s = (ab + ac + bc) / 2.0;
	out[0] = ab, out[1] = ac, out[2] = std::sqrt(s * (s - ab) * (s - ac) * (s - bc)), out[3] = exact_reciprocal(out[2]);
}
// Records `text` as the last error of `ctx` (or of the calling thread when ctx is null) and returns `status`.
rmd_status fail(rmd_context *ctx, rmd_status status, const std::string &text);
// The same for a caller that must not throw (the catch blocks of `guarded`): when even the message cannot be stored the status still comes back.
rmd_status fail_noexcept(rmd_context *ctx, rmd_status status, const char *what, const char *text) noexcept;
// "Nothing throws or aborts across the boundary" (include/raymond_hip.h): every extern "C" entry point that allocates with throwing containers
// (std::vector, std::string) runs its body through this — std::bad_alloc becomes RMD_ERR_OUT_OF_MEMORY, anything else RMD_ERR_HIP with the
// exception's text; the caller's process (a Rust or ctypes host) is never terminated by an unwinding C++ exception.
template <class F>
rmd_status guarded(rmd_context *ctx, const char *what, F &&body) noexcept {
	try {
		return body();
	} catch (const std::bad_alloc &) {
		return fail_noexcept(ctx, RMD_ERR_OUT_OF_MEMORY, what, "the host ran out of memory");
	} catch (const std::exception &e) {
		return fail_noexcept(ctx, RMD_ERR_HIP, what, e.what());
	} catch (...) {
		return fail_noexcept(ctx, RMD_ERR_HIP, what, "unknown exception");
	}
}
// Every rect lies inside the frame (64-bit sums: left + width may pass 2^32), and what a call says when one does not
constexpr const char *kRectOutside = "tile rectangle outside the framebuffer";
static inline bool rects_inside(const rmd_tile_rect *rects, uint32_t n_rects, uint32_t width, uint32_t height) {
	for (uint32_t i = 0; i < n_rects; i++)
		if ((uint64_t)rects[i].left + rects[i].width > width || (uint64_t)rects[i].top + rects[i].height > height) return false;
	return true;
}
// Whether any two of the byte ranges overlap; a null pointer is no range.  128-bit sums: a range may end past 2^64
struct Range {
	const void *at;
	unsigned __int128 bytes;
};
static inline bool any_overlap(std::initializer_list<Range> ranges) {
	for (const Range *i = ranges.begin(); i != ranges.end(); i++)
		for (const Range *j = i + 1; j != ranges.end(); j++) {
			const unsigned __int128 a = (uintptr_t)i->at, b = (uintptr_t)j->at;
			if (i->at && j->at && a < b + j->bytes && b < a + i->bytes) return true;
		}
	return false;
}
#ifdef RMD_WITH_HIP
// What an entry point does with its context first (api.cpp): "null context", or the context's device made current.
rmd_status bind(rmd_context *ctx);
// Rects inside the frame and pairwise disjoint (api_denoise.cpp); *why: the rule that was broken, the caller puts its own name in front
bool denoise_rects_ok(const rmd_tile_rect *rects, uint32_t n_rects, uint32_t width, uint32_t height, const char **why);
// After a wait for the context's stream: RMD_ERR_DEVICE_FAULT (and the fault words cleared) when a wave of a launch reported one, else RMD_OK.
rmd_status check_fault(rmd_context *ctx);
RenderParams make_params(const rmd_context *ctx, const rmd_scene *scene, const rmd_camera *cam, const rmd_settings *st);
bool primary_cull_allowed(const RenderParams &P);
// RenderParams::primary_cull of a launch whose own half holds: bit 0 the candidate sets, bit 1 the tile classes (primary_candidates.hpp)
inline uint32_t primary_cull_bits(bool regular, uint32_t n_grids, int64_t axis_pairs_tunable) {
	if (!regular || n_grids != 0u) return 0u;
	return axis_pairs_tunable == 0 ? 3u : axis_pairs_tunable == 3 ? 1u : 0u;
}
// RenderParams::end_black_paths of a launch (make_params has the argument): TRACE never ends a zero-throughput path, END always, flags 0 only where it is exact
inline bool end_black_paths_rule(uint32_t flags, bool has_scene, uint32_t n_grids, bool regular, bool on_plane) {
	return (flags & RMD_RENDER_TRACE_BLACK_PATHS) ? false : ((flags & RMD_RENDER_END_BLACK_PATHS) || !has_scene || (n_grids == 0u && regular && !on_plane));
}
// Does the camera lie on (or within 1e-9 of) one of the planes?  planes: origin and normal, six numbers each (api.cpp)
bool camera_on_a_plane(const std::vector<double> &planes, const rmd_camera *cam);
// The role-sorted spheres kernel's two-part work list (api.cpp, beside choose_split; work_list.hpp has the mapping the kernel shares)
WorkPlan plan_work_list(uint32_t wave_slots, uint32_t n_tiles, uint32_t sample_count, uint32_t k_uniform, uint32_t min_samples = kTailMinSamples,
                        uint32_t tail_x2 = kTailTilesPerSlotX2, uint32_t tail_parts = kTailParts, uint32_t n_tail_forced = 0u);
WorkPlan context_work_plan(const rmd_context *ctx, bool has_grid, uint32_t n_tiles, uint32_t sample_count, uint32_t pass_samples);
// The host half of rmd_scene_create (api_scene.cpp), also for the host-only probe of the primary rays' candidate sets (probe.cpp)
struct SceneObjects {
	std::vector<DevObject> objs;
	bool regular = true;
	uint32_t axis_pairs = 0;
	AxisWalls walls[3] = {};
	unsigned long long visit_mask = 0ull, grid_mask = 0ull;
};
rmd_status derive_scene_objects(rmd_context *ctx, const rmd_object *objects, uint32_t n_objects, uint32_t n_grids, int64_t axis_pairs_tunable, SceneObjects &out);
#endif
} // namespace rmd
