/*
 * raymond_hip.h — C-ABI of the MI355X-native radiance integrator.
 *
 * This library replaces ONE seam of Nyrox/raymond: the per-tile body of the
 * worker loop in `render_tiled`
 *
 *     reference  src/trace.rs:197-205   for y in tile rows { for x in tile cols {
 *                                           primary = generate_primary_ray(x, y, cam)   (:322-333 / :335-360)
 *                                           sample  = trace(primary, &context, 1)       (:232-320)
 *                                           tile.data[..] += sample } }
 *
 * Everything below that loop (Scene::intersect core/src/scene.rs:54-74, the
 * primitives core/src/geometry/primitives/{sphere,plane,triangle,aabb}.rs, the DDA grid walk
 * core/src/geometry/acc_grid.rs:89-185, the BRDF and samplers
 * src/trace.rs:362-416) runs inside one HIP kernel for gfx950.  Everything
 * above it (tile queue, progressive passes, TaskHandle, tone-map, file IO)
 * stays with the host.  There is no reference FFI for this path (the reference
 * has no `extern "C"` anywhere); the entry points below are what a cgo-style
 * Rust `extern "C"` block for that seam would bind — INTEGRATION.md shows the
 * Rust side.
 *
 * Conventions: plain C, POD structs, caller owns every buffer it passes, the
 * library owns the opaque handles.  Every function returns rmd_status
 * (0 = OK); nothing throws or aborts across the boundary — every entry point
 * that allocates on the host runs behind a catch: std::bad_alloc comes back as
 * RMD_ERR_OUT_OF_MEMORY (tests/test_abi.py forces it) — (the reference's
 * failure mode is a Rust panic — and a hang: `TaskHandle::await` polls a counter
 * that a panicked worker never decrements, src/trace.rs:82-92; here it is a
 * status + rmd_last_error()).  That holds inside the kernel too: every loop of
 * the render kernel has a bound that no input reaches, and a wave that runs
 * into one sets a device fault word, stops the launch handing out work and
 * leaves; the host then returns RMD_ERR_DEVICE_FAULT instead of a frame.
 * A context is thread-compatible (one calling thread at a time per handle).
 * All arithmetic is IEEE binary64, as in the reference (core/src/math.rs:10).
 */
#ifndef RAYMOND_HIP_H
#define RAYMOND_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMD_ABI_VERSION 6u

typedef int32_t rmd_status;
enum {
	RMD_OK = 0,
	RMD_ERR_INVALID_ARGUMENT = 1, /* null pointer, zero size, out-of-range index            */
	RMD_ERR_NO_DEVICE = 2,        /* HIP runtime present but no usable gfx950 device         */
	RMD_ERR_HIP = 3,              /* a HIP call failed; text in rmd_last_error               */
	RMD_ERR_OUT_OF_MEMORY = 4,
	RMD_ERR_GRID_INDEX = 5,       /* grid build hit the reference's out-of-bounds panic (Q5) */
	RMD_ERR_UNSUPPORTED = 6,      /* e.g. bounce_limit above RMD_MAX_BOUNCE_LIMIT            */
	RMD_ERR_RCCL = 7,
	RMD_ERR_DEVICE_FAULT = 8      /* a loop of the render kernel ran past its bound (it cannot, for any input: an internal fault);
	                                 the launch was cut short, the frame it wrote to is NOT valid; text in rmd_last_error.
	                                 Reported by the first call that waits for the launch (rmd_render_tiles,
	                                 rmd_context_synchronize, rmd_last_kernel_ms, rmd_framebuffer_download[_tiles],
	                                 rmd_framebuffer_upload_tiles, rmd_context_wait_transfers, rmd_resolve_tonemap,
	                                 rmd_resolve_tonemap_tiles, rmd_luminance_histogram_tiles, rmd_despike, rmd_despike_dual, rmd_tile_luma_error, rmd_tile_weighted_error,
	                                 rmd_reduce_framebuffer, rmd_render_tiles_moments, rmd_tile_error,
	                                 rmd_denoise, rmd_render_features, rmd_render_ids, rmd_ids_matte, rmd_render_ao, rmd_ao_resolve, rmd_denoise_guided, rmd_denoise_dual,
	                                 rmd_denoise_atrous_dual, rmd_denoise_atrous_dual_region,
	                                 rmd_tile_error_dual, rmd_tile_weighted_error_dual, rmd_denoise_dual_region, rmd_denoise_dual_guided,
	                                 rmd_denoise_guided_slope, rmd_denoise_dual_guided_slope,
	                                 rmd_denoise_dual_guided_slope_region, rmd_denoise_dual_select_slope,
	                                 rmd_denoise_atrous_slope, rmd_denoise_atrous_dual_slope,
	                                 rmd_denoise_atrous_dual_slope_region,
	                                 rmd_denoise_dual_guided_region, rmd_denoise_dual_select, rmd_denoise_atrous) */
};

/* ---- scene description (mirrors core/src/scene.rs:8-45, core/src/lib.rs:21-26) ---- */

/* enum Geometry { Plane, Sphere, Grid }  — core/src/scene.rs:9-13 (same order) */
enum { RMD_GEOM_PLANE = 0, RMD_GEOM_SPHERE = 1, RMD_GEOM_GRID = 2 };
/* enum Material { Diffuse, Metal, Emission } — core/src/lib.rs:21-26 (same order) */
enum { RMD_MAT_DIFFUSE = 0, RMD_MAT_METAL = 1, RMD_MAT_EMISSION = 2 };

/* Material::Diffuse(color, roughness) | Metal(color, roughness) | Emission(e, v2, f1, f2).
 * For Emission `color` carries the first vector (the only field trace() reads,
 * src/trace.rs:250-252); v2/f1/f2 ride along untouched in `emission_aux`.
 * |roughness| must be <= 512 for Diffuse/Metal (rmd_scene_create returns RMD_ERR_UNSUPPORTED
 * otherwise): the GGX sampling angle roughness^2 * sqrt(u / (1 - u)) is reduced on the device
 * by a method that is accurate below 2^45. */
typedef struct rmd_material {
	uint32_t kind;
	uint32_t _pad;
	double color[3];
	double roughness;
	double emission_aux[5];
} rmd_material;

/* One scene::Object (core/src/scene.rs:33-37).  Object order is significant:
 * Scene::intersect keeps the FIRST object on distance ties (strict '<', :61). */
typedef struct rmd_object {
	uint32_t geometry_kind;
	uint32_t grid_index; /* RMD_GEOM_GRID: index into the grids array           */
	double origin[3];    /* Plane.origin (plane.rs:6) / Sphere.origin (sphere.rs:6) */
	double normal[3];    /* Plane.normal (plane.rs:7)                            */
	double radius;       /* Sphere.radius (sphere.rs:7)                          */
	rmd_material material;
} rmd_object;

/* One AccGrid (core/src/geometry/acc_grid.rs:27-33) in the compact layout:
 * `cells[c]` = offset into `mapping_table`; `mapping_table[off]` = count,
 * followed by `count` triangle indices (acc_grid.rs:67-74), both as u32
 * instead of usize.  Triangles are split SoA-by-role: positions (read by every
 * Möller-Trumbore test, triangle.rs:11-44) and vertex normals (read only on a
 * shaded hit, triangle.rs:47-68) instead of the 264-byte AoS Triangle.
 * All pointers are HOST pointers; rmd_scene_create copies them to HBM. */
typedef struct rmd_grid_desc {
	double bbox_min[3]; /* mesh.bounding_box.min (mesh.rs:123-140)      */
	double bbox_max[3];
	uint32_t resolution[3]; /* acc_grid.rs:6-17                          */
	uint32_t _pad;
	double cell_size[3]; /* acc_grid.rs:38                               */
	const uint32_t *cells;
	uint64_t n_cells; /* = res.x*res.y*res.z                            */
	const uint32_t *mapping_table;
	uint64_t n_mapping;
	const double *tri_pos; /* n_tris * 9: v0.xyz v1.xyz v2.xyz          */
	const double *tri_nrm; /* n_tris * 9: n0.xyz n1.xyz n2.xyz          */
	uint64_t n_tris;
	const struct rmd_grid_build *built; /* NULL, or the rmd_grid_build these pointers belong to (set by rmd_grid_build_describe): rmd_scene_create
	                                       then derives its device tables ONCE per build (about 50 ms of host time for 100k triangles) and
	                                       every later upload of the same grid — one per render_tiled call and GPU — reuses them.
	                                       The pointer is only as good as the build: a caller that COPIES a description, or hands its arrays
	                                       to another owner, and lets the copy outlive rmd_grid_build_destroy must set `built` to NULL in
	                                       the copy (the arrays then only have to stay valid for the duration of rmd_scene_create, as in
	                                       ABI 3).  A struct that was zero-initialised and filled by hand has NULL here.                  */
} rmd_grid_desc;

/* CameraSettings (src/trace.rs:32-40) + Transform (src/transform.rs:4-7, position only). */
typedef struct rmd_camera {
	uint32_t backbuffer_width;
	uint32_t backbuffer_height;
	double fov_vert; /* degrees */
	double position[3];
	double focal_length;
	double aperture_radius; /* CameraSettings.aperture_radius.  The reference's worker always calls the pinhole
	                           generate_primary_ray (:199, :322-333) whatever this field holds — its thin-lens
	                           generate_primary_ray_with_dof (:335-360) is never called — and so does this library
	                           unless rmd_settings.flags carries RMD_RENDER_DOF (and the radius is > 0: with
	                           radius 0 the reference's rejection loop never terminates). */
} rmd_camera;

#define RMD_MAX_BOUNCE_LIMIT 16u

/* The part of Settings (src/trace.rs:42-55) the per-tile body reads, plus the
 * RNG definition the reference lacks (it uses the unseedable thread_rng). */
#define RMD_RENDER_DOF 1u /* rmd_settings.flags: primary rays through generate_primary_ray_with_dof (an extension: the
                             reference defines that function but its render loop never calls it) */
/* Paths whose throughput has become exactly (0, 0, 0) — a diffuse bounce off a black surface ((1 - F)(1 - metal) (.) (0,0,0), src/trace.rs:279-281),
 * a GGX sample below the surface (geometry_smith's max(n.l, 0), :373).  trace() multiplies whatever the rest of such a path finds by that zero
 * (:281-282, :315-318), so its sample is exactly (0, 0, 0) in the reference too — unless a LATER vertex of the path produces a non-finite
 * radiance, because 0 x NaN = NaN.  The one source of such a vertex is the interpolated normal of a mesh hit (triangle.rs:47-68: Heron's
 * radicand rounding below zero for a hit on an edge, or vertex normals that sum to zero); a scene of planes and spheres has none.
 *
 *   flags = 0 (default)               REFERENCE-IDENTICAL on every scene.  Such paths are ended early only where that is PROVED not to
 *                                     change a sample: in scenes WITHOUT grid objects whose parameters are all REGULAR — every coordinate,
 *                                     colour and radiance finite and at most 1e150 in magnitude, no sphere of radius 0, no material of
 *                                     roughness 0 (rmd_scene_create decides this once per scene).  Everywhere else — a scene with a grid,
 *                                     or a grid-less scene outside that class: an Emission((inf, 0, 0)) behind a black bounce is
 *                                     0 x inf = NaN, roughness 0 makes geometry_schlick_ggx 0 / 0 (:372-378) — every path is traced to its
 *                                     end, the last depth included, as the reference does, so a sample that is NaN in the reference is NaN
 *                                     here (tests/test_gpu_parity.py::test_flags_0_is_reference_identical_for_non_finite_scene_parameters).
 *                                     What is NOT covered: events of probability ~2^-53 per path inside the regular class (r1 = 0 exactly
 *                                     in a diffuse pdf, a bounce ray exactly opposite to the view vector).
 *                                     This is what a drop-in caller gets (integration/gpu.rs).
 *   RMD_RENDER_END_BLACK_PATHS        opt-in, scenes with grids: end such paths there too.  Every sample that is finite in the reference
 *                                     keeps its value bit for bit; a sample the reference makes NaN behind a zero weight comes out (0, 0, 0)
 *                                     (how many pixels of the benchmark frames that is: DESIGN.md section 3, counted on the GPU).  A
 *                                     quarter to a third fewer path segments.
 *   RMD_RENDER_TRACE_BLACK_PATHS      never end a path early, grid or not (measurement and tests: the reference's full segment count).
 * END and TRACE together are refused (RMD_ERR_INVALID_ARGUMENT).  The rule itself: tests/test_gpu_parity.py::test_black_path_modes_*. */
#define RMD_RENDER_TRACE_BLACK_PATHS 2u
#define RMD_RENDER_END_BLACK_PATHS 4u
typedef struct rmd_settings {
	uint32_t bounce_limit; /* Settings.bounce_limit; trace() starts at depth 1 (:200,:235) */
	uint32_t sample_begin; /* first sample index s of this pass                             */
	uint32_t sample_count; /* number of consecutive samples to add per pixel               */
	uint32_t flags;        /* 0 or RMD_RENDER_DOF | one of RMD_RENDER_{TRACE,END}_BLACK_PATHS   */
	uint64_t seed; /* Philox key; see "RNG" below                                   */
} rmd_settings;

/* core::tile::Tile geometry (core/src/tile.rs:7-14) without the sample buffer. */
typedef struct rmd_tile_rect {
	uint32_t left, top, width, height;
} rmd_tile_rect;

/*
 * RNG (replaces rand::random::<f64>() at src/trace.rs:260,287,288,326,327,340,341,397,398).
 * Counter-based Philox4x32-10 (Salmon et al., SC'11), key = (seed lo32, seed hi32).  A sample's random numbers come
 * in BLOCKS: block b of sample s of pixel p is the Philox output for counter (p = y*W + x, s, b, 0), four words w0..w3:
 *     u_first  = (((uint64)w1 << 32 | w0) >> 11) * 2^-53        53-bit uniforms in [0,1), as rand 0.6 makes an f64
 *     u_second = (((uint64)w3 << 32 | w2) >> 11) * 2^-53
 *     u_22     = ((w0 & 0x7FF) << 11 | (w2 & 0x7FF)) * 2^-22     the 22 bits those two conversions discard
 * Every consumer takes exactly one block, in the order the reference makes its calls within a sample:
 *     block 0               pixel jitter: x <- u_first, y <- u_second (:326-327)
 *     then, thin lens only  one block per round of the rejection loop: r1 <- u_first, r2 <- u_second (:340-341)
 *     then                  one block per shaded depth: r1 <- u_first, r2 <- u_second (:397-398 or :287-288), and
 *                           r (:260) <- u_22 of the sample's PREVIOUS block (the jitter block or the last lens round for the first
 *                           depth, the preceding depth's block afterwards).  r only decides diffuse against specular: it is compared
 *                           with prob_d, which is 0.5 for Diffuse and 0.0 for Metal (:263-264), and for those two values a 22-bit
 *                           uniform gives exactly the probabilities a 53-bit one does.  Taking it from the previous block makes a
 *                           hit's lobe known when the hit is: a diffuse bounce off a black surface can end its path (see
 *                           RMD_RENDER_END_BLACK_PATHS) without the depth's block ever being drawn.  (Since ABI 2; ABI 1 took r from
 *                           the depth's own block: same distribution, different samples.  ABI 3 changed no sample, only which
 *                           rmd_settings.flags value ends black paths in scenes with grids; ABI 4 changed no sample either: it added
 *                           RMD_ERR_DEVICE_FAULT, rmd_reduce_framebuffer_async, rmd_launch_info.waves_per_workgroup and the rule for
 *                           non-finite scene parameters below; ABI 5 changed no sample: rmd_launch_info.queued, RMD_TUNE_PATH_QUEUES,
 *                           and every allocating entry point behind a catch; ABI 6 changed no sample: it added the per-pixel second
 *                           moments — rmd_render_tiles_moments[_async] — and rmd_tile_error.)
 * (One Philox evaluation per path segment, and no RNG state beyond a block counter and those 22 bits.)
 */

typedef struct rmd_context rmd_context;
typedef struct rmd_scene rmd_scene;
typedef struct rmd_comm rmd_comm;

/* ---- lifetime ---- */
/* RMD_ABI_VERSION of the library that was LOADED.  The structs of this header have grown from version to version (rmd_grid_desc::built in 4,
 * rmd_launch_info::queued in 5): a caller compiled against another version must compare this with its own RMD_ABI_VERSION before its first other
 * call and refuse to go on when they differ (raymond_amd/lib.py and integration/gpu.rs do). */
uint32_t rmd_abi_version(void);
/* One context per GPU (device_ordinal = HIP device index).  Creates its own stream. */
rmd_status rmd_context_create(int32_t device_ordinal, rmd_context **out);
/* Same, but launches on a caller-owned hipStream_t (passed as void*, 0 = null stream). */
rmd_status rmd_context_create_on_stream(int32_t device_ordinal, void *hip_stream, rmd_context **out);
void rmd_context_destroy(rmd_context *ctx);
/* Text of the last failure on this context (or of the last failed context-less call when ctx = NULL). */
const char *rmd_last_error(const rmd_context *ctx);

/* Scheduling tunables of a context.  NONE of them changes a result — every setting renders the same frame bit for bit
 * (tests/test_gpu_parity.py checks that) — they only move work between waves.  Defaults are read from the environment
 * variable named beside each key ONCE, when the context is created; 0 / unset = the library's own choice. */
enum {
	RMD_TUNE_SAMPLE_SPLIT = 0, /* RMD_SAMPLE_SPLIT: waves a wave tile's sample range is split over (0 = automatic)  */
	RMD_TUNE_WALK_BATCH = 1,   /* RMD_WALK_BATCH: lanes of a wave that wait for a grid walk before one is run        */
	RMD_TUNE_MASK_BUDGET = 2,  /* RMD_MASK_BUDGET: LDS bytes for the grids' occupancy masks (read by rmd_scene_create) */
	RMD_TUNE_LAUNCH_FORM = 3,  /* RMD_LAUNCH_FORM: 0 = the library's choice: persistent workgroups, one per CU, whose waves draw work
	                              items from a counter — launches with fewer items than the device has wave slots as one wave per
	                              item; 1 / "per-item" = always one wave per item; 2 / "persistent" = always persistent workgroups */
	RMD_TUNE_SCRATCH_CAP_MB = 4, /* RMD_SCRATCH_CAP_MB: cap of the per-sample scratch of split launches, MiB (0 = an eighth of the
	                              device memory that is free when the buffer is (re)allocated); a launch whose samples do not fit —
	                              or whose buffer the device cannot provide — runs as several passes                       */
	RMD_TUNE_WALK_CUT = 5,     /* RMD_WALK_CUT: K + 1, where a grid-walk call of a wave stops stepping under its last K rays and leaves their
	                              walks to the wave's next call (0 = the library's choice, K = 7; 1 = every call finishes every walk)      */
	RMD_TUNE_SPLIT_MIN_SAMPLES = 6, /* RMD_SPLIT_MIN_SAMPLES: fewest samples per pixel a work item of a split launch may hold (0 = the library's
	                              choice: 4 in scenes with grids — two items per wave tile from 4 samples per pixel on — 64 without)      */
	RMD_TUNE_CHAIN_ITEMS = 7,  /* RMD_CHAIN_ITEMS: split launches of scenes with grids whose persistent waves draw their next work item while the last
	                              paths of the current one finish: 0 = the library's choice (every such launch), 1 = never,                     
	                              2 = always                                                                                                  */
	RMD_TUNE_AXIS_PAIRS = 8,   /* RMD_AXIS_PAIRS: read by rmd_scene_create — pairs of opposite planes whose normals are exactly +e_k / -e_k (the walls of an
	                              axis-aligned room) tested with one component of the ray: 0 = the library's choice (yes, in scenes of regular
	                              parameters — and, in such a scene without a grid, a launch without the thin lens gives the generation trips of the
	                              spheres kernel their own candidate sets: the spheres and the one pair their tile's primary rays can hit),
	                              1 = never (every pair takes the general test, no candidate sets), 2 = the pairs as for 0, no candidate sets,
	                              3 = as 0 without the tile classes (work items whose tile sees one emitting or one black wall: every item is general).
	                              Same samples, bit for bit, whatever the value                                                              */
	RMD_TUNE_PATH_QUEUES = 9,  /* RMD_PATH_QUEUES: persistent split launches of scenes with grids keep their paths in queues in device memory — ray
	                              compaction between bounces: a wave's trips are 64 new samples, 64 parked hits or one grid walk for 64 parked rays
	                              (rmd_launch_info.queued): 0 = the library's choice (yes), 1 = never (a lane keeps its path: same samples, bit for bit) */
	RMD_TUNE_COUNT = 10
};
/* Free and total memory of the context's device, bytes (hipMemGetInfo): what a host that shares the GPU sizes its launches by. */
rmd_status rmd_context_memory_info(rmd_context *ctx, uint64_t *out_free_bytes, uint64_t *out_total_bytes);
rmd_status rmd_context_set_tunable(rmd_context *ctx, uint32_t key, int64_t value);
rmd_status rmd_context_get_tunable(const rmd_context *ctx, uint32_t key, int64_t *out_value);

/* Uploads the object table and the grids to HBM.  Replaces the per-worker
 * `scene.clone()` (src/trace.rs:182-185): one resident copy per GPU. */
rmd_status rmd_scene_create(rmd_context *ctx, const rmd_object *objects, uint32_t n_objects,
                            const rmd_grid_desc *grids, uint32_t n_grids, rmd_scene **out);
void rmd_scene_destroy(rmd_scene *scene);

/* ---- device buffers for hosts without their own HIP binding ---- */
rmd_status rmd_framebuffer_alloc(rmd_context *ctx, uint32_t width, uint32_t height, double **out_dev); /* zeroed W*H*3 */
rmd_status rmd_framebuffer_free(rmd_context *ctx, double *dev);
rmd_status rmd_framebuffer_zero(rmd_context *ctx, double *dev, size_t n_doubles);
rmd_status rmd_framebuffer_download(rmd_context *ctx, const double *dev, double *host, size_t n_doubles);
rmd_status rmd_framebuffer_upload(rmd_context *ctx, const double *host, double *dev, size_t n_doubles);

/* Tile rectangles of a device framebuffer <-> a PACKED host buffer: rect i's pixels row-major, width * height * 3 doubles, one rect after the
 * other in the order of `rects` — the layout of core::tile::Tile.data (core/src/tile.rs:13).  What a host scheduler needs to keep the tile sums
 * resident on the device between progressive passes and move only the tiles a message needs (TileProgressed / TileFinished, src/trace.rs:211-219)
 * instead of the whole W * H * 3 frame up and down around every call.  Rects must lie inside the W x H frame.
 * _async: the tiles are packed on the context's stream (behind the renders enqueued before), copied on the context's COPY stream — renders
 * enqueued afterwards overlap the copy — and are in `host_packed` once rmd_context_wait_transfers has returned; `host_packed` should be pinned
 * memory (rmd_host_alloc) for the copy to be asynchronous.  At most two such downloads are in flight per context: a third waits for the first. */
rmd_status rmd_framebuffer_download_tiles(rmd_context *ctx, const double *dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                                          uint32_t n_rects, double *host_packed);
rmd_status rmd_framebuffer_download_tiles_async(rmd_context *ctx, const double *dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                                                uint32_t n_rects, double *host_packed);
rmd_status rmd_context_wait_transfers(rmd_context *ctx);
rmd_status rmd_framebuffer_upload_tiles(rmd_context *ctx, const double *host_packed, double *dev, uint32_t width, uint32_t height,
                                        const rmd_tile_rect *rects, uint32_t n_rects);
/* Page-locked host memory (hipHostMalloc): copies to and from it run at the link's rate and asynchronously. */
rmd_status rmd_host_alloc(rmd_context *ctx, size_t bytes, void **out_host);
rmd_status rmd_host_free(rmd_context *ctx, void *host); /* ctx may be NULL (a block may outlive the context it was allocated through) */

/*
 * The hot path.  For every pixel (x,y) of every rect in `tiles`:
 *     accum[(x + y*W)*3 + c] += sample(x,y,s).c   for s = sample_begin .. sample_begin+sample_count-1, in that order
 * i.e. `sample_count` consecutive executions of src/trace.rs:197-205 over those
 * tiles.  Dividing by the sample count stays with the caller (TaskHandle::await,
 * src/trace.rs:95).  `accum_dev` is a DEVICE pointer to W*H*3 doubles, row-major
 * RGB (x + y*W, the layout await() assembles, :97).  Rects must lie inside the
 * backbuffer and must not overlap each other within one call.
 * Synchronous: returns after the kernel has completed.
 */
rmd_status rmd_render_tiles(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera,
                            const rmd_settings *settings, const rmd_tile_rect *tiles, uint32_t n_tiles,
                            double *accum_dev);
/* Same, enqueue only; pair with rmd_context_synchronize (lets one host thread drive several GPUs). */
rmd_status rmd_render_tiles_async(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera,
                                  const rmd_settings *settings, const rmd_tile_rect *tiles, uint32_t n_tiles,
                                  double *accum_dev);
rmd_status rmd_context_synchronize(rmd_context *ctx);
/*
 * The same render that also accumulates each pixel's SECOND MOMENT (since ABI 6).  `accum_sq_dev` is a second DEVICE buffer laid out like
 * `accum_dev` (W*H*3 doubles, row-major RGB); for every pixel of every rect and every channel c:
 *     accum   [i] += L_s.c          for s = sample_begin .. sample_begin+sample_count-1, in that order   (exactly as rmd_render_tiles)
 *     accum_sq[i] += L_s.c * L_s.c  the same samples in the same order; the product rounded, then added (no fused multiply-add)
 * Both sums are the same bits whatever form the launch takes (direct or buffered, any split, persistent or one wave per item, queued, chained,
 * any number of scratch passes), and two calls over [0, k) and [k, n) give the bits of one call over [0, n).  accum_sq_dev = NULL is exactly
 * rmd_render_tiles[_async]; accum_sq_dev == accum_dev is RMD_ERR_INVALID_ARGUMENT.  rmd_framebuffer_alloc / _zero / _download_tiles /
 * _upload_tiles serve the second buffer like the first.
 */
rmd_status rmd_render_tiles_moments(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                                    const rmd_tile_rect *tiles, uint32_t n_tiles, double *accum_dev, double *accum_sq_dev);
rmd_status rmd_render_tiles_moments_async(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                                          const rmd_tile_rect *tiles, uint32_t n_tiles, double *accum_dev, double *accum_sq_dev);
/*
 * Per-tile noise estimate from the two sums after n = sample_count samples.  For each pixel and channel, with S = accum, Q = accum_sq:
 *     m = S / n;   v = (Q - S*m) / (n - 1), set to 0 if negative;   e_c = sqrt(v / n) / max(|m|, floor)
 *     e_pixel = max_c e_c       (+inf if any S or Q of the pixel is not finite, or n < 2)
 *     out_err_host[r] = the largest e_pixel over rect r's pixels   (0 for a rect without pixels)
 * — the relative standard error of the pixel's mean, worst channel, worst pixel: one firefly keeps its tile's error high.  Rects may have any
 * size and must lie inside the W x H frame; `floor` must be finite and > 0; accum_sq_dev == accum_dev is RMD_ERR_INVALID_ARGUMENT.
 * Synchronous (waits for the renders enqueued before it on the context; reports a device fault of one of them like rmd_context_synchronize).
 */
rmd_status rmd_tile_error(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height,
                          uint32_t sample_count, double floor, const rmd_tile_rect *rects, uint32_t n_rects, double *out_err_host);
/*
 * Denoises a frame from its two sums: non-local means with the variance-normalised patch distance of Rousselle, Knaus and Zwicker, "Adaptive
 * Rendering with Non-Local Means Filtering" (SIGGRAPH Asia 2012).  An addition within ABI 6: RMD_ABI_VERSION stays 6, no struct or entry point
 * changes, and a caller finds the function by its symbol.
 * S = accum_dev, Q = accum_sq_dev (W*H*3 doubles each, row-major RGB, as rmd_render_tiles_moments writes them); pixel i of rect j holds
 * n_i = rect_sample_counts[j] samples, a pixel that no rect covers n_i = 0.  For pixel i and channel c:
 *     u_ic = S_ic / n_i;   v_ic = max(0, (Q_ic - S_ic*u_ic) / (n_i - 1)) / n_i      (the variance of the mean, as rmd_tile_error)
 *     pixel i is VALID if n_i >= 2 and its six S and Q values are finite
 *     term_c(a, b) = ((u_ac - u_bc)^2 - alpha*(v_ac + min(v_ac, v_bc))) / (eps + k^2*(v_ac + v_bc)),   eps = 1e-10, k^2 = k*k
 * For a valid p and a neighbour q = p + d with |d_x|, |d_y| <= radius, q inside the frame (not clamped) and valid: for every patch offset o with
 * |o_x|, |o_y| <= patch_radius, a = clamp(p + o), b = clamp(q + o) (clamped to the frame: the border pixel repeats); the three terms at o are
 * taken if a and b are both valid, summed over c in order 0, 1, 2.
 *     D(p, q) = (sum of the taken terms) / (3 * the number of offsets taken)     — the centre offset is always taken
 *             the offsets summed row by row (o_x ascending), then the row sums over o_y ascending
 *     w(p, q) = exp(-max(0, D(p, q)))                                             — w(p, p) = 1 for alpha >= 0
 *     out_pc  = sum_q w(p,q)*u_qc / sum_q w(p,q)     q in raster order (d_y, then d_x, ascending), for a valid p
 *     out_pc  = S_pc / n_p                           exactly as IEEE gives it, for a p that is not valid (a NaN stays NaN)
 * A pixel that is not valid is never a neighbour or a patch term, so a NaN does not spread.  out_dev holds MEANS, not sums:
 * rmd_resolve_tonemap(out_dev, sample_count = 1) tone-maps it.  radius = 0 gives S / n bit for bit.
 * Arguments (all checked before the device is touched): 0 <= radius <= 12, 0 <= patch_radius <= 4, k finite and > 0, alpha finite and >= 0;
 * width, height > 0; accum_dev, accum_sq_dev and out_dev non-NULL, and no two of the three W*H*3-double ranges overlap; rects and
 * rect_sample_counts are HOST arrays of n_rects entries (non-NULL when n_rects > 0); every rect lies inside the frame and no two overlap.
 * Anything else is RMD_ERR_INVALID_ARGUMENT.  Synchronous (waits for the renders enqueued before it on the context; reports a device fault of
 * one of them like rmd_context_synchronize).  Defaults a caller may start from: radius 10, patch_radius 3, k 0.45, alpha 1 (DESIGN.md
 * section 11).
 */
rmd_status rmd_denoise(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height,
                       const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects,
                       uint32_t radius, uint32_t patch_radius, double k, double alpha, double *out_dev);
/*
 * FIRST-HIT FEATURE BUFFERS (an addition within ABI 6: RMD_ABI_VERSION stays 6, no struct changes; a caller finds the functions by their
 * symbols).  A feature buffer is W*H*RMD_FEATURE_CHANNELS doubles, pixel-interleaved: feat[(x + y*W)*7 + j], j = 0..2 the normal's x, y, z,
 * 3..5 the albedo's r, g, b, 6 the depth.  rmd_feature_buffer_alloc allocates one, zeroed; rmd_framebuffer_free / _zero / _download / _upload
 * take a pointer and a count of doubles and serve feature buffers as they are.
 * rmd_render_features: for every pixel i of every rect and s = sample_begin .. sample_begin + sample_count - 1, in that order, the PRIMARY RAY
 * exactly as rmd_render_tiles takes it for (pixel, s) — Philox block 0 for the jitter, and with RMD_RENDER_DOF (aperture_radius > 0) the lens'
 * rounds after it — is intersected with the scene once (Scene::intersect).  The sample's feature vector phi_s:
 *     hit on object o at distance t (frag = ro + rd*t):
 *         normal  plane: o.normal as stored (not normalised); sphere: normalize(frag - origin); grid: the interpolated normal of the hit triangle
 *                 at frag (it may be NaN, and then stays NaN) — the functions the shading calls, for every material kind, Emission included
 *         albedo  o.material.color (for Emission: the emitted radiance — a light's outline is an edge too)
 *         depth   t as Scene::intersect returns it
 *     miss, or a sample for which the thin lens yields no ray (the render's sample is zero there): seven zeros
 *     feat   [i*7+j] += phi_s.j
 *     feat_sq[i*7+j] += phi_s.j * phi_s.j      the product rounded, then added (no fused multiply-add)
 * — the contract of rmd_render_tiles_moments: calls over [0, k) and [k, n) give the bits of one call over [0, n), and the bits do not depend on
 * how the rects cut the frame.  bounce_limit and the black-path flags are ignored (RMD_RENDER_END_BLACK_PATHS and _TRACE_BLACK_PATHS together
 * are still refused).  feat_sq_dev = NULL skips the squares.  feat_dev NULL, feat_sq_dev == feat_dev, tiles NULL with n_tiles > 0, a rect outside
 * the frame or two rects that overlap are RMD_ERR_INVALID_ARGUMENT before the device is touched.  The pass does not change what
 * rmd_last_launch_info and rmd_last_kernel_ms report.  rmd_render_features waits for the launch like rmd_render_tiles and, like
 * every call that waits, returns RMD_ERR_DEVICE_FAULT if a render enqueued before it on the context reported one; the pass itself raises no
 * fault code: its own loop runs sample_count times, and the grid walk it calls is bounded by the rays' exit counters and has nothing to
 * report (the render loops' reports watch what a wave does BETWEEN walks, which this kernel does not have).  The _async form only enqueues.
 */
#define RMD_FEATURE_CHANNELS 7u /* 0..2 normal xyz, 3..5 albedo rgb, 6 depth */
rmd_status rmd_feature_buffer_alloc(rmd_context *ctx, uint32_t width, uint32_t height, double **out_dev); /* zeroed W*H*7 */
rmd_status rmd_render_features(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                               const rmd_tile_rect *tiles, uint32_t n_tiles, double *feat_dev, double *feat_sq_dev);
rmd_status rmd_render_features_async(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                                     const rmd_tile_rect *tiles, uint32_t n_tiles, double *feat_dev, double *feat_sq_dev);
/*
 * FIRST-HIT OBJECT IDS WITH COVERAGE, AND MATTES (an addition within ABI 6: RMD_ABI_VERSION stays 6, no struct changes; a caller finds the
 * functions by their symbols).  Which object a pixel shows, and how much of the pixel it covers.  A mean of object indices means nothing, so an
 * ID buffer is a small table per pixel: W*H*RMD_ID_WORDS uint32_t words, pixel-interleaved, the record of pixel i = x + y*W at ids[i*10 ..]:
 *     words 2j, 2j+1 (j = 0 .. RMD_ID_SLOTS-1)   key_j, count_j
 *     word 8                                      other
 *     word 9                                      samples
 * A key is 0 (an empty slot), o + 1 (object o, the index into rmd_scene_create's `objects`; for a grid object the grid object's own index) or
 * RMD_ID_MISS (a miss, or a sample for which the thin lens yields no ray: the class rmd_render_features turns into seven zeros).
 * The rule for one sample with key k: for j = 0, 1, 2, 3 in order — if key_j == k then count_j += 1 and stop; if key_j == 0 then key_j = k,
 * count_j = 1 and stop.  If no slot took it, other += 1.  Then samples += 1.  So the slots are in first-seen order, empty slots trail, and
 * sum(count_j) + other == samples.  Every count, `other` and `samples` are modulo 2^32.
 * A record is 40 bytes = 5 doubles: rmd_id_buffer_alloc allocates a zeroed buffer, and rmd_framebuffer_free / _zero / _download / _upload serve it
 * as they are with n_doubles = W*H*5.
 * rmd_render_ids: for every pixel of every rect and s = sample_begin .. sample_begin + sample_count - 1, in that order, the primary ray exactly as
 * rmd_render_features takes it (Philox block 0, then the lens' rounds under RMD_RENDER_DOF) is intersected with the scene once, and the rule is
 * applied with the hit's object, or with RMD_ID_MISS.  The contract is rmd_render_features': calls over [0, k) and [k, n) leave the words of one
 * call over [0, n), the words do not depend on how the rects cut the frame, and a pixel no rect covers keeps its words.  So is the rest: bounce_limit
 * and the black-path flags are ignored (both together are still refused); ids_dev NULL, tiles NULL with n_tiles > 0, a rect outside the frame or two
 * rects that overlap are RMD_ERR_INVALID_ARGUMENT, in that order, before the device is touched; a scene whose object table the launch cannot hold
 * is RMD_ERR_UNSUPPORTED with the buffer untouched; the pass does not change what rmd_last_launch_info and rmd_last_kernel_ms report; rmd_render_ids
 * waits like rmd_render_features and reports an earlier device fault as it does, the pass itself raises none; the _async form only enqueues.
 * rmd_ids_matte: `objects` (HOST memory, n_objects <= 2048) is a SET of object indices, RMD_ID_MISS standing for the background; duplicates are
 * allowed.  Per pixel, c = the sum, as a 64-bit integer, of count_j over the slots whose key is in the set; matte = (double)c / (double)samples, one
 * correctly rounded division, and 0.0 where samples == 0.  `other` is never counted — which objects it holds is unknown —, and
 * *other_pixels_host (may be NULL) receives the exact number of pixels with other != 0: at 0 the matte is exact.  Alpha is 1 - matte({RMD_ID_MISS}).
 * n_objects == 0 writes zeros.  RMD_ERR_INVALID_ARGUMENT before the device is touched, in this order: width or height 0; ids_dev or matte_dev NULL;
 * objects NULL with n_objects > 0; n_objects > 2048; an entry equal to 0xFFFFFFFE (its key would be RMD_ID_MISS); the two ranges overlapping; then a
 * NULL context.  The call waits; its scratch (the sorted distinct keys and one counter) stays on the context.
 */
#define RMD_ID_SLOTS 4u
#define RMD_ID_WORDS 10u /* key_0 count_0 .. key_3 count_3 other samples */
#define RMD_ID_MISS 0xFFFFFFFFu
rmd_status rmd_id_buffer_alloc(rmd_context *ctx, uint32_t width, uint32_t height, uint32_t **out_dev); /* zeroed W*H*10 words */
rmd_status rmd_render_ids(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                          const rmd_tile_rect *tiles, uint32_t n_tiles, uint32_t *ids_dev);
rmd_status rmd_render_ids_async(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                                const rmd_tile_rect *tiles, uint32_t n_tiles, uint32_t *ids_dev);
rmd_status rmd_ids_matte(rmd_context *ctx, const uint32_t *ids_dev, uint32_t width, uint32_t height, const uint32_t *objects, uint32_t n_objects,
                         double *matte_dev, uint64_t *other_pixels_host);
/*
 * AMBIENT OCCLUSION OF THE FIRST HIT, AS EXACT COUNTS (an addition within ABI 6: RMD_ABI_VERSION stays 6, no struct changes; a caller finds the
 * functions by their symbols).  How much of the hemisphere above the first hit is blocked within a distance: the contact shadows that none of
 * normal, albedo, depth or ID carries.  Each sample's outcome is one bit, so an AO buffer holds counts: W*H*RMD_AO_WORDS uint32_t words,
 * pixel-interleaved, the record of pixel i = x + y*W at ao[i*4 ..]:
 *     word 0   occluded
 *     word 1   open
 *     word 2   none
 *     word 3   samples
 * All four are modulo 2^32, and occluded + open + none == samples.  A record is 16 bytes = 2 doubles: rmd_ao_buffer_alloc allocates a zeroed
 * buffer, and rmd_framebuffer_free / _zero / _download / _upload serve it as they are with n_doubles = W*H*2.
 * rmd_render_ao: for every pixel of every rect and s = sample_begin .. sample_begin + sample_count - 1, in that order:
 *   1  the primary ray exactly as rmd_render_features takes it (Philox block 0, then the lens' rounds under RMD_RENDER_DOF) is intersected with
 *      the scene once.  A miss, or a sample the thin lens yields no ray for, does none += 1, samples += 1 and ends there.
 *   2  for a hit on object o at distance t: frag = ro + rd*t, and N is the normal rmd_render_features defines (the plane's as stored, the sphere's
 *      normalised, the grid's interpolated, possibly NaN).  The material is ignored: Emission and Metal included, the construction is the diffuse one.
 *   3  (r1, r2) = the first and second 53-bit uniform of the sample's NEXT Philox block: block 1 for the pinhole, block 1 + the lens' rounds
 *      otherwise — the block the render's first shaded depth draws.  The block's 22-bit uniform is not used.
 *   4  the bounce ray of trace()'s diffuse branch (src/trace.rs:261-269, 396-416): (T, B) = onb(N), l = cosine_hemisphere(r1, r2),
 *      dir = normalize(Matrix3::from_cols(T, N, B) * l), origin = frag + N * 0.00001.
 *   5  Scene::intersect(origin, dir) gives (o2, t2).  The sample is OCCLUDED if o2 is an object and t2 < max_distance; otherwise it is OPEN — a NaN
 *      t2, or a NaN ray that hits nothing, is open.  Then samples += 1.  The closest hit compared with max_distance is the definition.
 * The contract is rmd_render_features': calls over [0, k) and [k, n) leave the words of one call over [0, n), the words do not depend on how the
 * rects cut the frame, and a pixel no rect covers keeps its words.  So is the rest: bounce_limit and the black-path flags are ignored (both together
 * are still refused); the pass does not change what rmd_last_launch_info and rmd_last_kernel_ms report; rmd_render_ao waits like rmd_render_features
 * and reports an earlier device fault as it does, the pass itself raises none; the _async form only enqueues.  Refused before the device is touched,
 * in this order: scene, camera or settings NULL; ao_dev NULL, or tiles NULL with n_tiles > 0; max_distance not > 0 (NaN is refused; +inf is allowed
 * and means "any hit"); a rect outside the frame or two rects that overlap, then the context and the render arguments, as rmd_render_features does —
 * all RMD_ERR_INVALID_ARGUMENT; a scene whose object table the launch cannot hold is RMD_ERR_UNSUPPORTED with the buffer untouched.
 * rmd_ao_resolve writes W*H doubles: out = (double)open / (double)(open + occluded) — the sum a 64-bit integer, one correctly rounded division —,
 * and empty_value where open + occluded == 0; *empty_pixels_host (may be NULL) receives the exact number of such pixels.
 * RMD_ERR_INVALID_ARGUMENT before the device is touched, in this order: width or height 0; ao_dev or out_dev NULL; empty_value not finite; the two
 * ranges overlapping; then a NULL context.  The call waits; its scratch (one counter, 16 bytes) stays on the context.
 */
#define RMD_AO_WORDS 4u /* occluded open none samples */
rmd_status rmd_ao_buffer_alloc(rmd_context *ctx, uint32_t width, uint32_t height, uint32_t **out_dev); /* zeroed W*H*4 words */
rmd_status rmd_render_ao(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                         const rmd_tile_rect *tiles, uint32_t n_tiles, double max_distance, uint32_t *ao_dev);
rmd_status rmd_render_ao_async(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera, const rmd_settings *settings,
                               const rmd_tile_rect *tiles, uint32_t n_tiles, double max_distance, uint32_t *ao_dev);
rmd_status rmd_ao_resolve(rmd_context *ctx, const uint32_t *ao_dev, uint32_t width, uint32_t height, double empty_value, double *out_dev,
                          uint64_t *empty_pixels_host);
/*
 * CLOSEST-HIT QUERIES FOR CALLER-SUPPLIED RAYS (an addition within ABI 6: RMD_ABI_VERSION stays 6, no struct of an earlier version changes; a caller
 * finds the functions by their symbols).  The passes above answer "what does this pixel see" for rays the library makes itself; these answer it for
 * rays the caller hands in: picking, visibility between scene points, a pass of the caller's own built from hits.
 * A RAY is RMD_RAY_DOUBLES = 6 doubles: origin x y z, direction x y z.  The direction is used as given and never normalised; t is in units of it, as in
 * Scene::intersect (core/src/scene.rs:54-74).  Any bit pattern is allowed in any component.  A HIT is one rmd_ray_hit, 40 bytes = RMD_HIT_DOUBLES = 5
 * doubles, so the framebuffer helpers serve both kinds of buffer as they are (n_doubles = 6n and 5n): rmd_framebuffer_zero / _download / _upload,
 * and rmd_framebuffer_free, which frees any device block the library handed out — ray and hit buffers have no free call of their own, as ID and AO
 * buffers have none.
 * rmd_intersect_rays: for every i < n_rays, hits[i] is Scene::intersect on ray i — the closest hit over all objects, the comparison a strict '<', so
 * the lower index wins a tie — with the normal rmd_render_features defines at frag = origin + direction * t: a plane's stored normal as stored,
 * normalize(frag - centre) for a sphere, the interpolated triangle normal for a mesh (NaN included).  `triangle` is the grid's triangle index for a
 * mesh object and 0 otherwise.  A miss writes {0, {0, 0, 0}, -1, 0} in full: hit buffers compare byte for byte.  Nothing else is written; a ray's
 * record does not depend on n_rays, on the ray's index or on its neighbours.  rays_dev and hits_dev are device memory and must not overlap.
 * rmd_intersect_rays waits for the context's stream and reports an earlier device fault, as rmd_render_features does; the _async form only enqueues
 * (rmd_context_synchronize ends it).  rmd_intersect_rays_host is the convenience form on host memory — allocate, upload, call, download, free — and
 * gives the same bytes.  None of them changes what rmd_last_launch_info and rmd_last_kernel_ms report.
 * rmd_camera_rays writes, for every i < n_rays, the pinhole generate_primary_ray (src/trace.rs:322-333) of pixel (xy_host[2i], xy_host[2i + 1]) at the
 * jitter uniforms (uv_host[2i], uv_host[2i + 1]) to rays_dev[6i ..]; uv_host NULL means 0.5, 0.5 everywhere, the pixel's centre, bit for bit.  Only
 * position, fov_vert and the backbuffer size of the camera are read: there is no thin lens, whose rays need the sample's random stream.  Its output
 * feeds rmd_intersect_rays without leaving the device.  Synchronous.
 * Refused before the device is touched and with the buffers untouched, in this order:
 *   1  a NULL pointer — scene, rays, hits, out_dev, camera, xy_host —: RMD_ERR_INVALID_ARGUMENT.  A NULL ray, hit or xy buffer is allowed only
 *      when n_rays == 0;
 *   2  n_rays > RMD_MAX_RAYS (2^30: the batch index stays a uint32_t): RMD_ERR_INVALID_ARGUMENT;
 *   3  (rmd_camera_rays) a backbuffer width or height of 0 or above 65535, or a pixel outside the frame: RMD_ERR_INVALID_ARGUMENT;
 *   4  a NULL context, then the scene's own refusals as a render makes them: a scene of another context is RMD_ERR_INVALID_ARGUMENT, a scene whose
 *      object table and grid masks the launch cannot hold in a CU's LDS is RMD_ERR_UNSUPPORTED.
 * n_rays == 0 is success with no launch (after the refusals).  rmd_ray_buffer_alloc / rmd_hit_buffer_alloc hand out zeroed buffers for n_rays
 * rays (n_rays of 0 or above RMD_MAX_RAYS, or out_dev NULL: RMD_ERR_INVALID_ARGUMENT).
 */
#define RMD_RAY_DOUBLES 6u
#define RMD_HIT_DOUBLES 5u
#define RMD_MAX_RAYS (1ull << 30)
typedef struct rmd_ray_hit {
	double t;          /* distance of the closest hit; 0 on a miss */
	double normal[3];  /* the normal the shading would use there; zeros on a miss */
	int32_t object;    /* index into the scene's objects; -1 on a miss */
	uint32_t triangle; /* the grid's triangle index for a mesh object, else 0 */
} rmd_ray_hit;         /* 40 bytes */
rmd_status rmd_ray_buffer_alloc(rmd_context *ctx, uint64_t n_rays, double **out_dev);      /* zeroed n*6 doubles */
rmd_status rmd_hit_buffer_alloc(rmd_context *ctx, uint64_t n_rays, rmd_ray_hit **out_dev); /* zeroed n records */
rmd_status rmd_intersect_rays(rmd_context *ctx, const rmd_scene *scene, const double *rays_dev, uint64_t n_rays, rmd_ray_hit *hits_dev);
rmd_status rmd_intersect_rays_async(rmd_context *ctx, const rmd_scene *scene, const double *rays_dev, uint64_t n_rays, rmd_ray_hit *hits_dev);
rmd_status rmd_intersect_rays_host(rmd_context *ctx, const rmd_scene *scene, const double *rays_host, uint64_t n_rays, rmd_ray_hit *hits_host);
rmd_status rmd_camera_rays(rmd_context *ctx, const rmd_camera *camera, const uint32_t *xy_host, const double *uv_host, uint64_t n_rays, double *rays_dev);
/*
 * rmd_denoise with a FEATURE WEIGHT (Rousselle, Manzi and Zwicker, "Robust Denoising using Feature and Color Information", 2013; an addition
 * within ABI 6).  Everything rmd_denoise defines stays word for word (validity, D(p, q), w_c = exp(-max(0, D)), clamping, sum orders, the output
 * for a pixel that is not valid).  Added, with F = feat_dev, G = feat_sq_dev (feature buffers as rmd_render_features writes them) and n_i the
 * pixel's count as before, for j = 0..6:
 *     f_ij = F_ij / n_i;   g_ij = max(0, (G_ij - F_ij*f_ij) / (n_i - 1)) / n_i          (as u and v)
 *     pixel i is FEATURE-VALID if it is valid and its fourteen F and G values are finite
 *     s_ij = 1 for j = 0..5;   s_i6 = f_i6 * f_i6                  (depth is judged relative to the pixel's own depth)
 *     Phi_j(p, q) = ((f_pj - f_qj)^2 - (g_pj + min(g_pj, g_qj))) / (eps + k_f^2 * max(tau * s_pj, g_pj)),   eps = 1e-10, k_f^2 = k_f*k_f
 *     D_f = 0;  for j = 0..6:  if Phi_j > D_f then D_f = Phi_j     (a NaN Phi_j is skipped by the comparison)
 *     w_f = exp(-D_f)
 *     w(p, q) = w_f if p and q are both feature-valid and w_f < w_c, else w_c
 * and out is the w-weighted mean as before.  So w(p, p) = 1, a pixel whose mesh normal is NaN is filtered by colour alone, a miss never mixes
 * with a hit (Phi_6 = t^2 / eps), and two misses do.  The gradient term of the 2013 paper and its second filtering pass are left out on
 * purpose (of this call: rmd_denoise_guided_slope, further down, adds a form of the gradient term).  feat_dev = feat_sq_dev = NULL is
 * exactly rmd_denoise (k_f and tau are then not read), and rmd_denoise is that call.  Beyond
 * rmd_denoise's rules: one of the two NULL and the other not, k_f or tau not finite or not > 0, the two W*H*7-double feature ranges overlapping
 * each other or out_dev's range: RMD_ERR_INVALID_ARGUMENT before the device is touched.  Values a caller may start from: k_f 1.0, tau 1e-2 (the
 * best of the sweep in DESIGN.md section 12; the paper's 0.6 and 1e-3 filter less and measured worse on the two test scenes).  Synchronous, like rmd_denoise.
 */
rmd_status rmd_denoise_guided(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, const double *feat_dev, const double *feat_sq_dev,
                              uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects,
                              uint32_t radius, uint32_t patch_radius, double k, double alpha, double k_f, double tau, double *out_dev);
/*
 * A FAST filter for previews: the edge-avoiding a-trous wavelet filter of Dammertz, Sewtz, Hanika and Lensch ("Edge-Avoiding A-Trous Wavelet
 * Transform for fast Global Illumination Filtering", 2010), its weights steered by the per-pixel variance and by the feature buffers, the
 * variance carried from level to level as in the spatial part of SVGF (Schied et al. 2017).  An addition within ABI 6: RMD_ABI_VERSION stays 6,
 * no struct changes, a caller finds the function by its symbol.  `levels` passes of 5 x 5 taps at steps 1, 2, 4, ... : 25 * levels taps per pixel
 * against rmd_denoise's 441 neighbours of 49 patch terms each.
 * S, Q, F, G, the rects, n_i, u, v, VALID, f, g, FEATURE-VALID, s_ij, eps, k^2 and k_f^2 are rmd_denoise_guided's, word for word; there is one
 * count per rect, and it serves colour and features alike.
 *     state   c^0 = u and v^0 = v: three channels each, per pixel
 *     taps    H5 = {1/16, 1/4, 3/8, 1/4, 1/16};  h(i, j) = H5[i + 2] * H5[j + 2] for i, j in -2..2   (these products are exact in binary64)
 * Level l = 0 .. levels - 1, step s = 2^l, for a valid p: the taps are q = p + s*(i, j), in raster order (j ascending, then i ascending).  A tap
 * is taken if q lies inside the frame (not clamped) and q is valid; the centre tap is always taken, through the same operations as any other.
 *     term_c  rmd_denoise's formula with (u, v) read as (c^l, v^l) of p and q
 *     D       = ((term_0 + term_1) + term_2) / 3.0
 *     w_c     = exp(-(D > 0 ? D : 0))                    — a NaN D gives w_c = 1, as the comparison leaves it
 *     w       = w_f if feat_dev is given, p and q are both feature-valid and w_f < w_c, else w_c
 *               Phi_j, D_f and w_f = exp(-D_f) exactly rmd_denoise_guided's, made from f and g, which no level changes
 *     hw      = h(i, j) * w
 *     from 0.0, over the taken taps in order:   A_c = A_c + hw * c^l_qc;   B_c = B_c + (hw * hw) * v^l_qc;   Wsum = Wsum + hw
 *     c^{l+1}_pc = A_c / Wsum;    v^{l+1}_pc = B_c / (Wsum * Wsum)
 * For a p that is not valid, c and v are never read by anyone.
 *     out_pc  = c^levels_pc     for a valid p
 *     out_pc  = S_pc / n_p      exactly as IEEE gives it, for any other p (a NaN stays NaN)
 * out_dev holds MEANS, as rmd_denoise's.  So: levels = 0 gives S / n bit for bit; NULL features give the colour weight alone; all-zero features
 * with counts >= 2 give w_f = 1 and so the unguided bytes; a pixel that is not valid is never a tap, so a NaN does not spread; a pixel's value does
 * not depend on how the rects cut the frame.
 * The propagated v steers the later levels and is NOT an error estimate: after level 0 the neighbours' noise is correlated, and sqrt(mean v)
 * reads 4 - 5 times below the true error.  Because of that v is not returned.  There is no region form; the dual form is rmd_denoise_atrous_dual.
 * Arguments (all checked before the device is touched, anything else RMD_ERR_INVALID_ARGUMENT): rmd_denoise_guided's rules for the buffers, their
 * aliasing (the three W*H*3-double ranges, the two W*H*7-double feature ranges), width, height, the rects, the counts, k and alpha, and for k_f
 * and tau when features are given; feat_dev and feat_sq_dev are both given or both NULL (when NULL, k_f and tau are not read);
 * levels <= RMD_ATROUS_MAX_LEVELS.  Synchronous, and reports an earlier device fault, like rmd_denoise.  Values a caller may start from:
 * levels 5, k 3.0, alpha 1, k_f 1.0, tau 1e-2 (k = 0.45, rmd_denoise's, is useless here: a single pixel's distance has no patch to average
 * over).
 */
#define RMD_ATROUS_MAX_LEVELS 8u
rmd_status rmd_denoise_atrous(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, const double *feat_dev, const double *feat_sq_dev,
                              uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects,
                              uint32_t levels, double k, double alpha, double k_f, double tau, double *out_dev);
/*
 * DUAL-BUFFER denoising (the cross filter of Rousselle, Knaus and Zwicker 2012, the paper rmd_denoise follows; an addition within ABI 6:
 * RMD_ABI_VERSION stays 6, no struct changes, a caller finds the functions by their symbols).  The samples are split into two disjoint sets A
 * and B; each half is filtered with weights computed from the OTHER half, so that a weight never depends on the noise of the value it
 * multiplies, and the difference of the two filtered halves estimates the error of the frame that is delivered.
 * S_A = accum_a_dev, Q_A = accum_sq_a_dev, S_B = accum_b_dev, Q_B = accum_sq_b_dev (W*H*3 doubles each, as rmd_render_tiles_moments writes
 * them); pixel i of rect j holds n_Ai = rect_counts_a[j] samples in A and n_Bi = rect_counts_b[j] in B, a pixel no rect covers 0 and 0.
 *     u_A, v_A and the validity of half A are exactly rmd_denoise's u, v and VALID on (S_A, Q_A, n_A); likewise u_B, v_B for half B
 *     pixel i is DUAL-VALID if it is valid in both halves
 *     w_B(p, q) is rmd_denoise's w(p, q) word for word — D, clamping, the offsets taken, the sum orders, exp(-max(0, D)) — evaluated on
 *             (u_B, v_B) with "valid" read as dual-valid everywhere; w_A(p, q) the same on (u_A, v_A)
 * For a dual-valid p, q = p + d over the dual-valid neighbours inside the frame in raster order as in rmd_denoise:
 *     f_Ac(p) = sum_q w_B(p,q)*u_Aqc / sum_q w_B(p,q)          f_Bc(p) = sum_q w_A(p,q)*u_Bqc / sum_q w_A(p,q)
 *     out_pc  = (n_A*f_Ac + n_B*f_Bc) / (n_A + n_B)            the two products, their sum, one division (n_A + n_B is exact)
 *     h_c     = (f_Ac - f_Bc) / 2
 *     err_p   = (h_0*h_0 + h_1*h_1 + h_2*h_2) / 3              summed in channel order
 * For a p that is not dual-valid:
 *     out_pc  = (S_Apc + S_Bpc) / (n_A + n_B)                  exactly as IEEE gives it (a NaN stays NaN, 0 / 0 is NaN)
 *     err_p   = NaN
 * and such a pixel is never a neighbour or a patch term.  h_c is the one-degree-of-freedom estimate of the standard error of the delivered
 * mean: f_A and f_B are two estimates of the same value from disjoint samples, and half their difference has the variance of their mean
 * (for n_A = n_B).  It measures VARIANCE and not the filter's bias, which both halves share and which cancels in the difference — so it
 * reads LOW: on the test scene its per-tile RMS is about half the true error of the delivered frame.  It ranks
 * tiles; it is not a bound.  radius = 0 gives f_A = u_A and f_B = u_B bit for bit, so out and err are exact there.  With the two halves equal
 * (the same sums and counts) f_A = f_B = rmd_denoise of either half bit for bit and err = 0; out is then (n*f + n*f) / (2n), which is f
 * again bit for bit when n is a power of two and may differ from it in the last bit otherwise.
 * out_dev: W*H*3 MEANS, as rmd_denoise's.  err_dev: W*H doubles, or NULL when the estimate is not wanted.
 * Arguments (all checked before the device is touched): rmd_denoise's rules for radius, patch_radius, k, alpha, width, height and the rects;
 * the four sum buffers and out_dev non-NULL; no two of the six ranges (five of W*H*3 doubles, err_dev's W*H) overlap; rect_counts_a and
 * rect_counts_b are HOST arrays of n_rects entries, non-NULL when n_rects > 0.  Anything else is RMD_ERR_INVALID_ARGUMENT.  Synchronous, and
 * reports an earlier device fault, like rmd_denoise.  The feature weight of rmd_denoise_guided is not part of this call:
 * rmd_denoise_dual_guided adds it.
 */
rmd_status rmd_denoise_dual(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev,
                            const double *accum_sq_b_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *rect_counts_a,
                            const uint32_t *rect_counts_b, uint32_t n_rects, uint32_t radius, uint32_t patch_radius, double k, double alpha,
                            double *out_dev, double *err_dev);
/*
 * rmd_denoise_dual for SOME PIXELS of the frame (an addition within ABI 6, found by its symbol).  Everything rmd_denoise_dual defines stays word
 * for word: validity, dual validity, both weights, clamping, sum orders, out, err, the values of a pixel that is not dual-valid.  rects,
 * rect_counts_a and rect_counts_b describe the WHOLE frame as there — neighbours and patch terms come from anywhere in it.  Added:
 *     for every pixel inside a rect of `region`, out_dev and err_dev receive exactly the bytes rmd_denoise_dual would write there
 *     every other double of out_dev and err_dev is not written at all: whatever it held before the call it holds after
 * (the value of a pixel does not depend on how the frame is cut into workgroups: every sum order above is fixed per pixel).  So calls over
 * disjoint regions into the same buffers compose to rmd_denoise_dual's frame, in any order, and the cost of a call follows the region's
 * area.  `region` is a HOST array of n_region rects under the rules of `rects` — inside the frame, no two overlapping —,
 * of any size and alignment; it need not coincide with `rects`.  n_region = 0 (region may then be NULL), or a region without pixels, writes
 * nothing and returns RMD_OK; the call still waits and still reports an earlier device fault.  region NULL with n_region > 0, and every
 * failure of rmd_denoise_dual, is RMD_ERR_INVALID_ARGUMENT before the device is touched.  Synchronous, like rmd_denoise_dual.  rmd_denoise and
 * rmd_denoise_guided have no region form: nothing would call one.
 */
rmd_status rmd_denoise_dual_region(rmd_context *ctx,
    const double *accum_a_dev, const double *accum_sq_a_dev,
    const double *accum_b_dev, const double *accum_sq_b_dev,
    uint32_t width, uint32_t height,
    const rmd_tile_rect *rects, const uint32_t *rect_counts_a,
    const uint32_t *rect_counts_b, uint32_t n_rects,
    const rmd_tile_rect *region, uint32_t n_region,
    uint32_t radius, uint32_t patch_radius, double k, double alpha,
    double *out_dev, double *err_dev);
/*
 * rmd_denoise_dual with the FEATURE WEIGHT of rmd_denoise_guided (an addition within ABI 6, found by its symbol).  Everything rmd_denoise_dual
 * defines stays word for word: validity, dual validity, w_A, w_B, clamping, every sum order, out, err, the values of a pixel that is not
 * dual-valid.  Added, with F = feat_dev, G = feat_sq_dev (feature buffers as rmd_render_features writes them):
 *     pixel i of rect j holds n_Fi = rect_counts_f[j] feature samples, a pixel no rect covers 0.  The features are NOT split into halves:
 *     they carry their own count, so a caller may render them at any count (the render loops pass n_A + n_B)
 *     for j = 0..6:  f_ij = F_ij / n_Fi;   g_ij = max(0, (G_ij - F_ij*f_ij) / (n_Fi - 1)) / n_Fi
 *     pixel i is FEATURE-VALID if it is dual-valid, n_Fi >= 2 and its fourteen F and G values are finite
 *     s_ij, Phi_j(p, q), D_f and w_f = exp(-D_f) are exactly rmd_denoise_guided's: the same operations in the same order, the division by
 *             eps + k_f^2 * max(tau * s_pj, g_pj), a NaN Phi_j skipped by the comparison
 *     the weight of the pass that filters A:  w_f if p and q are both feature-valid and w_f < w_B(p, q), else w_B(p, q)
 *     the weight of the pass that filters B:  the same with w_A(p, q); the same w_f enters both passes
 * So the features cut a weight, never raise one; they are noise-free beside the colour (one first hit per sample) and are shared by both
 * halves, which keeps an edge that lies below the noise out of BOTH filtered halves: the bias that rmd_denoise_dual's err cannot see, because
 * both halves share it, is removed rather than estimated.  With the two halves equal and rect_counts_f equal to their
 * counts, f_A = f_B = rmd_denoise_guided of either half bit for bit and err = 0.  All-zero features with counts >= 2 give w_f = 1 for every pair
 * and hence rmd_denoise_dual's bytes.
 * feat_dev = feat_sq_dev = NULL is exactly rmd_denoise_dual (rect_counts_f, k_f and tau are then not read).  Beyond rmd_denoise_dual's rules:
 * one of the two NULL and the other not; with features present, rect_counts_f (a HOST array of n_rects entries) NULL while n_rects > 0, k_f or
 * tau not finite or not > 0, either W*H*7-double feature range overlapping the other or any of the six ranges of rmd_denoise_dual:
 * RMD_ERR_INVALID_ARGUMENT before the device is touched.  Values a caller may start from: k_f 1.0, tau 1e-2, as for rmd_denoise_guided.
 * Synchronous, and reports an earlier device fault, like rmd_denoise_dual.
 */
rmd_status rmd_denoise_dual_guided(rmd_context *ctx,
    const double *accum_a_dev, const double *accum_sq_a_dev,
    const double *accum_b_dev, const double *accum_sq_b_dev,
    const double *feat_dev, const double *feat_sq_dev,
    uint32_t width, uint32_t height,
    const rmd_tile_rect *rects, const uint32_t *rect_counts_a,
    const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects,
    uint32_t radius, uint32_t patch_radius, double k, double alpha, double k_f, double tau,
    double *out_dev, double *err_dev);
/*
 * rmd_denoise_dual_guided for SOME PIXELS of the frame: rmd_denoise_dual_region's rules unchanged, on rmd_denoise_dual_guided's definition.  For
 * every pixel inside a rect of `region`, out_dev and err_dev receive exactly the bytes rmd_denoise_dual_guided would write there; every other
 * double of the two is not written at all.  rects and the three count arrays describe the WHOLE frame.  n_region = 0 (region may then be NULL),
 * or a region without pixels, writes nothing and returns RMD_OK; the call still waits and still reports an earlier device fault.
 * feat_dev = feat_sq_dev = NULL is exactly rmd_denoise_dual_region (rect_counts_f, k_f and tau are then not read).  Every failure of
 * rmd_denoise_dual_region or of rmd_denoise_dual_guided is RMD_ERR_INVALID_ARGUMENT before the device is touched.  Synchronous.
 */
rmd_status rmd_denoise_dual_guided_region(rmd_context *ctx,
    const double *accum_a_dev, const double *accum_sq_a_dev,
    const double *accum_b_dev, const double *accum_sq_b_dev,
    const double *feat_dev, const double *feat_sq_dev,
    uint32_t width, uint32_t height,
    const rmd_tile_rect *rects, const uint32_t *rect_counts_a,
    const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects,
    const rmd_tile_rect *region, uint32_t n_region,
    uint32_t radius, uint32_t patch_radius, double k, double alpha, double k_f, double tau,
    double *out_dev, double *err_dev);
/*
 * PER-PIXEL CHOICE AMONG SEVERAL DUAL-BUFFER FILTERS by Stein's unbiased risk estimate (an addition within ABI 6, found by its symbol; after
 * Rousselle, Manzi and Zwicker 2013).  Whole-frame.  Every candidate i < n_cands is one parameter set of
 * rmd_denoise_dual (guided = 0: k, alpha; k_f and tau are not read) or of rmd_denoise_dual_guided (guided != 0: k, alpha, k_f, tau) at the
 * call's radius and patch_radius.  Counts, u, v, validity, dual validity, the feature planes and feature validity are those calls', word for word.
 *   Per candidate i.  f_A,i and f_B,i are exactly the two cross passes of that call.  The weights that filter half X are made from the OTHER half
 *   (and the features), so f_X,i(p) is linear in u_X and  g_X,i(p) = d f_X,i(p) / d u_X(p) = w(p, p) / sum_q w(p, q):  the weight the pass gives the
 *   offset (0, 0) — through the same operations as any other offset, the feature weight included; it is 1 whenever alpha >= 0 — divided by the pass's
 *   own sum of weights, the denominator of f_X,i(p).
 *   SURE of half X, with u, v that half's mean and variance of the mean, per channel c:
 *       d_c = f_X,i,c - u_c;   t_c = ((d_c * d_c) - v_c) + ((2 * v_c) * g_X,i)
 *       sure_X,i(p) = ((t_0 + t_1) + t_2) / 3
 *   an unbiased estimate of E (f_X,i - truth)^2, the bias included (err of rmd_denoise_dual sees the variance alone); it may be negative.
 *   SURE of the candidate:  sure_i(p) = ((n_A * sure_A,i) + (n_B * sure_B,i)) / (n_A + n_B), NaN at a pixel that is not dual-valid.
 *   Selection.  E_i(p) = the mean of sure_i over the dual-valid pixels of the (2*sure_window + 1)^2 window around p that lie inside the frame:
 *   0.0, then those pixels' values added in raster order (row by row, left to right), divided by their number.  win(p) = the lowest index i with
 *   the smallest E_i(p): i replaces the best so far only if E_i < E_best, or E_best is NaN and E_i is not; all NaN: 0.
 *   m_i(p) = (the dual-valid in-frame pixels q of the (2*select_window + 1)^2 window around p with win(q) = i) / (the dual-valid in-frame pixels of
 *   that window): two integer counts, converted to double, one division — exact fractions that sum to 1 up to rounding, whatever the order.
 *   Output, for a dual-valid p:  f_X(p)_c = m_0 * f_X,0,c, then + m_i * f_X,i,c for i = 1 .. n_cands - 1 in that order;
 *       out and err   rmd_denoise_dual's operations on f_A and f_B, word for word
 *       sure_dev[p]   m_0 * sure_0(p), then + m_i * sure_i(p) in index order
 *       win_dev[p]    win(p)
 *   any other p: out is the merged mean and err NaN as in rmd_denoise_dual, sure_dev[p] is NaN and win_dev[p] is 0xFFFFFFFF.
 * So n_cands = 1 gives m_0 = 1 and rmd_denoise_dual's (rmd_denoise_dual_guided's) out and err bit for bit; a candidate listed a second time never
 * wins (the first of equal minima does), its m is 0 and the outputs are those of the list without it.  sure_dev of one candidate alone is that
 * filter's per-pixel SURE: its frame mean estimates the filter's mean squared error (within x0.8 - 1.3 of the true RMSE
 * after the root, where err reads x0.2 - 0.55); per tile it is too noisy to rank tiles, which stays err's task.
 * cands: a HOST array.  err_dev (W*H doubles), sure_dev (W*H doubles) and win_dev (W*H uint32) may each be NULL.
 * Arguments, all checked before the device is touched, anything else RMD_ERR_INVALID_ARGUMENT: rmd_denoise_dual's rules for the sum buffers,
 * out_dev, err_dev, width, height, the rects, rect_counts_a / _b, radius and patch_radius; cands non-NULL and 1 <= n_cands <=
 * RMD_DENOISE_MAX_CANDIDATES; sure_window and select_window <= 5; every candidate's reserved = 0, its k and alpha under rmd_denoise_dual's
 * rules, and for a guided one k_f and tau under rmd_denoise_dual_guided's; feat_dev and feat_sq_dev both given or both NULL, under
 * rmd_denoise_dual_guided's aliasing rule; a guided candidate needs both, and rect_counts_f when n_rects > 0; sure_dev and win_dev overlap
 * no other range.  Features given without a guided candidate are not read.  Synchronous, and reports an earlier device fault, like rmd_denoise_dual.
 * Values a caller may start from: {k 0.45 unguided, k 1.0 guided with k_f 1.0 and tau 1e-2}, both windows 2.
 */
typedef struct rmd_denoise_candidate {
	double k, alpha, k_f, tau;
	uint32_t guided, reserved;
} rmd_denoise_candidate;
enum { RMD_DENOISE_MAX_CANDIDATES = 4 };
rmd_status rmd_denoise_dual_select(rmd_context *ctx,
    const double *accum_a_dev, const double *accum_sq_a_dev,
    const double *accum_b_dev, const double *accum_sq_b_dev,
    const double *feat_dev, const double *feat_sq_dev,
    uint32_t width, uint32_t height,
    const rmd_tile_rect *rects, const uint32_t *rect_counts_a,
    const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects,
    uint32_t radius, uint32_t patch_radius,
    const rmd_denoise_candidate *cands, uint32_t n_cands, uint32_t sure_window, uint32_t select_window,
    double *out_dev, double *err_dev, double *sure_dev, uint32_t *win_dev);
/*
 * The guided non-local-means filters with a FEATURE-SLOPE TERM (additions within ABI 6: RMD_ABI_VERSION stays 6, no struct changes, found by their
 * symbols).  A tight feature weight reads the change of a feature along a CURVED surface — a sphere's normal differs from pixel to pixel — as an edge
 * and takes away neighbours the pixel needs (DESIGN.md sections 12 and 21).  The 2013 paper answers with the feature's gradient in the denominator of
 * Phi_j; here it is the feature's own local slope, estimated so that a step does not count, times a scale in pixels (the scale is not the paper's).
 * `slope`: a double, finite and >= 0 — the number of pixels of a feature's local slope that is not an edge.  Everything of the call without the
 * suffix stays word for word.  Added, for a FEATURE-VALID pixel p = (x, y) and channel j, with f the call's own feature means:
 *     a_l = f_pj - f_(x-1,y)j      present if x >= 1 and (x-1, y) is feature-valid
 *     a_r = f_(x+1,y)j - f_pj      present if x + 1 < W and (x+1, y) is feature-valid
 *     a_u = f_pj - f_(x,y-1)j,  a_d = f_(x,y+1)j - f_pj      likewise for the rows y - 1 and y + 1 (y + 1 < H)
 *     h_j  = (a_l*a_l < a_r*a_r ? a_l*a_l : a_r*a_r)  if both are present, else 0.0          — the two-sided minimum: a slope that continues on both
 *     v_j  = the same from a_u and a_d                                                         sides counts, a step, which has a flat side, does not
 *     m_pj = (slope * slope) * (h_j + v_j)
 *     t    = max(tau * s_pj, g_pj)         exactly the comparison of rmd_denoise_guided (a > g ? a : g)
 *     if m_pj > t then t = m_pj            (a NaN m is skipped by the comparison)
 *     the denominator of Phi_j(p, .) = eps + k_f^2 * t
 * Phi_j's numerator, D_f, w_f, w and every sum order are unchanged.  FEATURE-VALID is each call's own: rmd_denoise_guided's for
 * rmd_denoise_guided_slope; rmd_denoise_dual_guided's (dual-valid, n_F >= 2, fourteen finite values) for the dual calls.  So:
 *     slope = 0 gives the bytes of the call without the suffix, launches nothing more and takes no more scratch;
 *     features that are constant on one side of every pixel, on each axis, give those bytes at any slope (a step edge stays an edge, and
 *     "a miss never mixes with a hit" holds for every miss that has another miss beside it: its depth then has a flat side);
 *     a pixel on the frame's border, or beside a pixel that is not feature-valid, has no slope on that axis;
 *     the slope only raises a denominator: w_f rises towards w_c, never above it.
 * rmd_denoise_guided_slope             = rmd_denoise_guided with `slope` after tau
 * rmd_denoise_dual_guided_slope        = rmd_denoise_dual_guided with `slope` after tau; the same m enters both passes
 * rmd_denoise_dual_guided_slope_region = rmd_denoise_dual_guided_region likewise: for every pixel of the region, byte for byte what
 *                                        rmd_denoise_dual_guided_slope writes there; nothing else is written (the slopes are made over the whole frame)
 * rmd_denoise_dual_select_slope        = rmd_denoise_dual_select with cand_slopes after cands: a HOST array of n_cands doubles, candidate i's slope, read
 *                                        for guided candidates only; NULL = every slope 0 = rmd_denoise_dual_select exactly
 * feat_dev = feat_sq_dev = NULL behaves as in the call without the suffix, and `slope` is then not read.  With features, a slope (of a guided
 * candidate: cand_slopes[i]) that is not finite or is negative is RMD_ERR_INVALID_ARGUMENT before the device is touched, after the checks of k_f
 * and tau; every other rule, and its order, is that of the call without the suffix.  Synchronous, and they report an earlier device fault, like those.
 * The a-trous filters have their own _slope forms, right below.  Values a caller may start from: slope 3 at k_f 1.0, tau 1e-2.
 */
rmd_status rmd_denoise_guided_slope(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, const double *feat_dev, const double *feat_sq_dev,
                                    uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects,
                                    uint32_t radius, uint32_t patch_radius, double k, double alpha, double k_f, double tau, double slope, double *out_dev);
rmd_status rmd_denoise_dual_guided_slope(rmd_context *ctx,
    const double *accum_a_dev, const double *accum_sq_a_dev,
    const double *accum_b_dev, const double *accum_sq_b_dev,
    const double *feat_dev, const double *feat_sq_dev,
    uint32_t width, uint32_t height,
    const rmd_tile_rect *rects, const uint32_t *rect_counts_a,
    const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects,
    uint32_t radius, uint32_t patch_radius, double k, double alpha, double k_f, double tau, double slope,
    double *out_dev, double *err_dev);
rmd_status rmd_denoise_dual_guided_slope_region(rmd_context *ctx,
    const double *accum_a_dev, const double *accum_sq_a_dev,
    const double *accum_b_dev, const double *accum_sq_b_dev,
    const double *feat_dev, const double *feat_sq_dev,
    uint32_t width, uint32_t height,
    const rmd_tile_rect *rects, const uint32_t *rect_counts_a,
    const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects,
    const rmd_tile_rect *region, uint32_t n_region,
    uint32_t radius, uint32_t patch_radius, double k, double alpha, double k_f, double tau, double slope,
    double *out_dev, double *err_dev);
rmd_status rmd_denoise_dual_select_slope(rmd_context *ctx,
    const double *accum_a_dev, const double *accum_sq_a_dev,
    const double *accum_b_dev, const double *accum_sq_b_dev,
    const double *feat_dev, const double *feat_sq_dev,
    uint32_t width, uint32_t height,
    const rmd_tile_rect *rects, const uint32_t *rect_counts_a,
    const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects,
    uint32_t radius, uint32_t patch_radius,
    const rmd_denoise_candidate *cands, const double *cand_slopes, uint32_t n_cands, uint32_t sure_window, uint32_t select_window,
    double *out_dev, double *err_dev, double *sure_dev, uint32_t *win_dev);
/*
 * The guided A-TROUS filters with the same FEATURE-SLOPE TERM (additions within ABI 6: RMD_ABI_VERSION stays 6, no struct changes, found by their
 * symbols).  rmd_denoise_atrous, rmd_denoise_atrous_dual and rmd_denoise_atrous_dual_region (their definitions stand with their declarations) use
 * rmd_denoise_guided's Phi_j word for word, and a level-l tap lies up to 2 * 2^l pixels away: on a curved mirror every level but the first loses all
 * its taps to the normal term.  Each _slope call is the call without the suffix with `double slope` after tau; everything of
 * that call stays word for word.  Added, for a FEATURE-VALID pixel p and channel j, with f the call's own feature means:
 *     m_pj = (slope * slope) * (h_j + v_j)    exactly the m_pj above: per axis the two-sided minimum of the squared differences to the two neighbours at
 *                                             ONE pixel's distance, whatever the level; a neighbour is present if it is inside the frame and feature-valid
 *     t    = max(tau * s_pj, g_pj)            exactly the comparison of the call without the suffix (a > g ? a : g)
 *     if m_pj > t then t = m_pj               (a NaN m is skipped by the comparison)
 *     the denominator of Phi_j(p, .) = eps + k_f^2 * t
 * FEATURE-VALID is each call's own: rmd_denoise_atrous's for rmd_denoise_atrous_slope; the dual calls' (dual-valid, n_F >= 2, fourteen finite values)
 * for the other two.  The SAME m serves EVERY LEVEL and, in the dual calls, BOTH HALVES: the features do not change from level to level, so m is made
 * once.  It is deliberately NOT scaled by the level's step 2^l: `slope` is a distance in pixels, and a term that grew with the step would forgive every
 * curved surface at every level and undo the feature weight.  On a curved surface the unscaled term leaves the first one or two levels open and closes
 * the later ones; a larger slope opens more levels.  So, all bit for bit:
 *     slope = 0 gives the bytes of the call without the suffix, launches nothing more and takes no more scratch;
 *     feat_dev = feat_sq_dev = NULL behaves as in the call without the suffix, and `slope` is then not read (a NaN is accepted);
 *     features that are constant on one side of every pixel, on each axis, give the slope-0 bytes at any slope;
 *     features that are zero everywhere, at counts >= 2, give the bytes of the call without features;
 *     levels = 0 is the closed form of the call without the suffix (no feature and no slope is read);
 *     equal halves with rect_counts_f equal to their counts give rmd_denoise_atrous_slope's bytes and err = 0;
 *     rmd_denoise_atrous_dual_slope_region writes, for every pixel of the region, the bytes rmd_denoise_atrous_dual_slope writes there, and nothing else;
 *     calls over disjoint regions compose, and a pixel's value does not depend on how the rects cut the frame.
 * The region form makes m on the pixels its levels are computed on only (level 0's needed set), from the f it has made one pixel further out; a
 * neighbour's presence is still "inside the FRAME and feature-valid".  Its scratch stays on the context.
 * With features, a slope that is not finite or is negative is RMD_ERR_INVALID_ARGUMENT ("NAME: slope must be finite and >= 0") before the device is
 * touched, after the checks of k_f and tau; every other rule, its order and its text are those of the call without the suffix, with the name alone
 * differing.  Synchronous, and they report an earlier device fault, like those.  A value a caller may start from: slope 3 at k_f 1.0, tau 1e-2.
 */
rmd_status rmd_denoise_atrous_slope(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, const double *feat_dev, const double *feat_sq_dev,
                                    uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects,
                                    uint32_t levels, double k, double alpha, double k_f, double tau, double slope, double *out_dev);
rmd_status rmd_denoise_atrous_dual_slope(rmd_context *ctx,
    const double *accum_a_dev, const double *accum_sq_a_dev,
    const double *accum_b_dev, const double *accum_sq_b_dev,
    const double *feat_dev, const double *feat_sq_dev,
    uint32_t width, uint32_t height,
    const rmd_tile_rect *rects, const uint32_t *rect_counts_a,
    const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects,
    uint32_t levels, double k, double alpha, double k_f, double tau, double slope,
    double *out_dev, double *err_dev);
rmd_status rmd_denoise_atrous_dual_slope_region(rmd_context *ctx,
    const double *accum_a_dev, const double *accum_sq_a_dev,
    const double *accum_b_dev, const double *accum_sq_b_dev,
    const double *feat_dev, const double *feat_sq_dev,
    uint32_t width, uint32_t height,
    const rmd_tile_rect *rects, const uint32_t *rect_counts_a,
    const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects,
    const rmd_tile_rect *region, uint32_t n_region,
    uint32_t levels, double k, double alpha, double k_f, double tau, double slope,
    double *out_dev, double *err_dev);
/*
 * rmd_denoise_atrous on TWO SAMPLE HALVES, each filtered with the weights of the other, with rmd_denoise_dual's error estimate: the fast filter in
 * a form that can drive adaptive sampling (an addition within ABI 6: RMD_ABI_VERSION stays 6, no struct changes, found by its symbol).
 * S_A, Q_A, S_B, Q_B, the rects, n_A, n_B, u_A, v_A, u_B, v_B, validity and DUAL-VALID are rmd_denoise_dual's, word for word.  F, G, rect_counts_f,
 * n_F, f, g and FEATURE-VALID (dual-valid, n_F >= 2, fourteen finite values; the features carry their own count) are rmd_denoise_dual_guided's.
 * s_ij, Phi_j, D_f and w_f = exp(-D_f) are rmd_denoise_guided's.  H5, h(i, j), the tap order (j ascending, then i ascending), "inside the frame, not
 * clamped", term_c and D = ((term_0 + term_1) + term_2) / 3.0 are rmd_denoise_atrous's.
 *     state   c_A^0 = u_A, v_A^0 = v_A, c_B^0 = u_B, v_B^0 = v_B
 * Level l = 0 .. levels - 1, step 2^l, for a dual-valid p and a tap q that is taken (inside the frame and dual-valid; the centre tap is always
 * taken, through the same operations as any other):
 *     w_cB    = exp(-(D_B > 0 ? D_B : 0))                with D_B made from (c_B^l, v_B^l) of p and q
 *     w_B     = w_f if feat_dev is given, p and q are both feature-valid and w_f < w_cB, else w_cB
 *     hw_B    = h(i, j) * w_B
 *     from 0.0, over the taken taps in order:   A_c = A_c + hw_B * c_A^l_qc;   B_c = B_c + (hw_B * hw_B) * v_A^l_qc;   Wsum = Wsum + hw_B
 *     c_A^{l+1}_pc = A_c / Wsum;    v_A^{l+1}_pc = B_c / (Wsum * Wsum)
 * and symmetrically w_A, made from (c_A^l, v_A^l), filters half B.  The same w_f enters both.
 *     f_A = c_A^levels, f_B = c_B^levels; out and err are rmd_denoise_dual's operations on f_A and f_B, word for word
 * A pixel that is not dual-valid takes the merged mean (S_A + S_B) / (n_A + n_B) and err = NaN, and is never a tap.
 * So: levels = 0 gives f_A = u_A and f_B = u_B bit for bit, rmd_denoise_dual's radius-0 closed form.  With the two halves equal and rect_counts_f
 * equal to their counts, f_A = f_B = rmd_denoise_atrous of either half bit for bit and err = 0; out is then f again when n is a power of two.
 * NULL features give the colour weights alone (rect_counts_f, k_f and tau are then not read); all-zero features at counts >= 2 give the unguided
 * bytes.  A pixel's value does not depend on how the rects cut the frame.
 * err measures VARIANCE, not bias, and after level 0 the two halves' weights are no longer independent of the values they multiply: level l + 1
 * makes w_B from c_B^{l+1}, which level l made under weights from half A.  It therefore reads LOW.  It ranks tiles; it is not a bound (DESIGN.md
 * section 18).  The region form is rmd_denoise_atrous_dual_region: a level's taps reach two steps of 2^l pixels, so its cost follows the region dilated by
 * 2 * (2^levels - 1) pixels rather than the region.
 * Arguments (all checked before the device is touched, anything else RMD_ERR_INVALID_ARGUMENT): rmd_denoise_dual_guided's rules for the buffers,
 * their aliasing, the rects, the three count arrays, k, alpha, k_f and tau; levels <= RMD_ATROUS_MAX_LEVELS; err_dev may be NULL.  Synchronous,
 * and reports an earlier device fault, like rmd_denoise_dual.  Values a caller may start from: rmd_denoise_atrous's.
 */
rmd_status rmd_denoise_atrous_dual(rmd_context *ctx,
    const double *accum_a_dev, const double *accum_sq_a_dev,
    const double *accum_b_dev, const double *accum_sq_b_dev,
    const double *feat_dev, const double *feat_sq_dev,
    uint32_t width, uint32_t height,
    const rmd_tile_rect *rects, const uint32_t *rect_counts_a,
    const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects,
    uint32_t levels, double k, double alpha, double k_f, double tau,
    double *out_dev, double *err_dev);
/*
 * rmd_denoise_atrous_dual for SOME PIXELS of the frame (an addition within ABI 6: RMD_ABI_VERSION stays 6, no struct changes, found by its symbol).
 * Everything rmd_denoise_atrous_dual defines stays word for word.  rects and the three count arrays describe the WHOLE frame as there — taps come from
 * anywhere in it.  `region` is a HOST array of n_region rects under rmd_denoise_dual_region's rules: inside the frame, no two overlapping, of any size
 * and alignment; it need not coincide with `rects`.  Added:
 *     for every pixel inside a rect of `region`, out_dev and err_dev receive exactly the bytes rmd_denoise_atrous_dual would write there
 *     every other double of out_dev and err_dev is not written at all: whatever it held before the call it holds after
 * (every sum order above is fixed per pixel, so a pixel's value does not depend on which other pixels are computed).  Calls over disjoint regions
 * into the same buffers compose to rmd_denoise_atrous_dual's frame, in any order.  What is computed: the last level on the region; level l on the set
 * level l + 1 is computed on, dilated by 2 * 2^(l+1) pixels each way (a tap of level l + 1 reaches two steps of 2^(l+1)) and clipped to the frame; u, v, f
 * and g on level 0's set dilated by 2 — the region dilated by 2 * (2^levels - 1) in all.  No kernel but the memset and the painting of the count images
 * runs over the whole frame, so the cost follows that dilated area: 14 pixels each way at 3 levels, 62 at 5.  The call's scratch
 * memory is kept on the context and grown when a call needs more, not allocated per call; it is released with the context.
 * levels = 0 is the closed form on the region's pixels.  NULL features and err_dev = NULL behave as in rmd_denoise_atrous_dual.  n_region = 0 (region may
 * then be NULL), or a region without pixels, writes nothing and returns RMD_OK; the call still waits and still reports an earlier device fault.
 * Arguments (all checked before the device is touched, anything else RMD_ERR_INVALID_ARGUMENT): rmd_denoise_atrous_dual's rules; region non-NULL when
 * n_region > 0; every region rect inside the frame; no two region rects overlapping.  Synchronous, like rmd_denoise_atrous_dual.
 */
rmd_status rmd_denoise_atrous_dual_region(rmd_context *ctx,
    const double *accum_a_dev, const double *accum_sq_a_dev,
    const double *accum_b_dev, const double *accum_sq_b_dev,
    const double *feat_dev, const double *feat_sq_dev,
    uint32_t width, uint32_t height,
    const rmd_tile_rect *rects, const uint32_t *rect_counts_a,
    const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects,
    const rmd_tile_rect *region, uint32_t n_region,
    uint32_t levels, double k, double alpha, double k_f, double tau,
    double *out_dev, double *err_dev);
/*
 * Per-tile error of the delivered frame from rmd_denoise_dual's err_dev (W*H doubles):
 *     out_err_host[r] = sqrt((sum of err_p over rect r's pixels) / the rect's pixel count)
 * +inf if any err_p of the rect is NaN (a pixel that is not dual-valid), 0 for a rect without pixels.  An ABSOLUTE root mean square in
 * linear radiance — not relative like rmd_tile_error —, and low by what rmd_denoise_dual says of err.  Sum order: with the rect's pixels
 * numbered row-major, partial sum t (0 <= t < 256) adds pixels t, t + 256, t + 512, ... in that order; the 256 partial sums are then added
 * pairwise in halving steps (t with t ^ 32, ^ 16, ... ^ 1 within each group of 64, then the four groups as (g0 + g1) + (g2 + g3)).  Rects
 * as in rmd_tile_error: any size, inside the W x H frame.  err_dev NULL, width or height 0, rects or out_err_host NULL with n_rects > 0:
 * RMD_ERR_INVALID_ARGUMENT.  Synchronous, like rmd_tile_error.
 */
rmd_status rmd_tile_error_dual(rmd_context *ctx, const double *err_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects, uint32_t n_rects,
                               double *out_err_host);
/* Host-buffer convenience for a caller that keeps Tile.data in RAM, as the
 * reference does: upload accum, render, download (PCIe-inclusive). */
rmd_status rmd_render_tiles_host(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *camera,
                                 const rmd_settings *settings, const rmd_tile_rect *tiles, uint32_t n_tiles,
                                 double *accum_host);
/* Duration of the most recent render kernel on this context, from HIP events
 * recorded on the context's stream around the launch (valid after a sync). */
rmd_status rmd_last_kernel_ms(rmd_context *ctx, float *out_ms);
/* How the most recent render on this context was launched (tests assert that a comparison exercised the instantiation they mean). */
typedef struct rmd_launch_info {
	uint32_t passes;          /* launches of the render kernel (the per-sample scratch may force several)                           */
	uint32_t split_k;         /* work items per wave tile of the last pass; > 1 = pooled (pixel, sample) hand-out + ordered sum    */
	uint32_t persistent;      /* 1 = persistent workgroups drawing work items from a counter, 0 = one wave per work item — the form
	                             the last pass was actually LAUNCHED in (a scene whose object table and masks leave a persistent
	                             workgroup too little LDS runs as one wave per item whatever was asked for)                       */
	uint32_t end_black_paths; /* 1 = zero-throughput paths were ended (see RMD_RENDER_END_BLACK_PATHS)                             */
	uint32_t has_grid;        /* 1 = the grid instantiation (wave-cooperative DDA walk) ran                                         */
	uint32_t waves_per_workgroup; /* waves of a workgroup of the last pass (persistent form: 16 unless the LDS left room for fewer) */
	uint32_t buffered;        /* 1 = the pooled (pixel, sample) hand-out + per-sample scratch + ordered sum ran (split_k > 1, or one item per
	                             wave tile: short launches of scenes with grids), 0 = direct mode (lane = pixel, no scratch)               */
	uint32_t chained;         /* 1 = persistent waves drew their next work item while the last paths of the current one finished (short
	                             split launches of scenes with grids; RMD_TUNE_CHAIN_ITEMS)                                                */
	uint32_t queued;          /* 1 = the paths lived in per-wave queues in device memory and every trip of a wave served lanes that all needed
	                             the same thing (persistent split launches of scenes with grids; RMD_TUNE_PATH_QUEUES; ABI 5)            */
} rmd_launch_info;
rmd_status rmd_last_launch_info(const rmd_context *ctx, rmd_launch_info *out);

/* ---- output stage (TaskHandle::await src/trace.rs:93-99, cli_old/src/main.rs:155-181) ---- */
/* out_rgb8[i] = trunc(255 * (1 - exp(-(accum[i]/sample_count) * exposure))^(1/gamma)); device in, host out.  A pixel with a channel that is
 * NaN or outside (-1, 256) stays (0, 0, 0), as cast::<u8>() returning None leaves it (:176-181).  Byte for byte what the host's libm gives:
 * the device evaluates every pixel and the few whose value lies within 1e-7 of a truncation boundary are recomputed on the host. */
rmd_status rmd_resolve_tonemap(rmd_context *ctx, const double *accum_dev, uint32_t width, uint32_t height,
                               uint32_t sample_count, double exposure, double gamma, uint8_t *out_rgb8_host);
/* The same stage over tile rectangles, each at its own sample count, into a PACKED host buffer of bytes: rect j's pixels row-major, width_j *
 * height_j * 3 bytes, one rect after the other in the order of `rects` — rmd_framebuffer_download_tiles's layout in bytes.  What a render loop needs
 * to show the frame while it renders: live tiles at the current count, tiles that finished early at theirs, one tile's 8-bit pixels without the frame's.
 * For a pixel of rect j and channel c: s = accum_dev's sum — plus accum2_dev's, in one rounded addition, when accum2_dev is not NULL (a dual-buffer
 * render's two halves; the count is then n_A + n_B) —, p = s / (double)rect_sample_counts[j], and the byte is rmd_resolve_tonemap's, with the same
 * contract: byte for byte what the host's libm gives.  A count of 0 is allowed (zero sums: 0 / 0, a black pixel).  Rects may have any size and
 * alignment inside the width x height frame and may overlap; a rect without pixels contributes no bytes; n_rects = 0 writes nothing and returns RMD_OK.
 * RMD_ERR_INVALID_ARGUMENT, checked before the device is touched and with the output untouched: accum_dev NULL, width or height 0, rects or
 * rect_sample_counts NULL with n_rects > 0, out NULL while the rects hold pixels, a rect outside the frame, accum2_dev overlapping accum_dev.
 * RMD_ERR_UNSUPPORTED: more than 2^32 - 1 packed pixels.  Synchronous; reports an earlier device fault like rmd_resolve_tonemap.  The cost follows
 * the packed pixels, whatever the number and shape of the rects; the call's device scratch stays on the context and grows on demand. */
rmd_status rmd_resolve_tonemap_tiles(rmd_context *ctx, const double *accum_dev, const double *accum2_dev, uint32_t width, uint32_t height,
                                     const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects, double exposure, double gamma,
                                     uint8_t *out_rgb8_host_packed);

/* ---- automatic exposure: the luminance histogram of a frame and the exposure it asks for (no reference counterpart; the reference's exposure is 1) ---- */
#define RMD_LUMA_BINS 256u
/* Counts of pixels by luminance Y, binned by Y's IEEE binary64 bits alone: with E the unbiased exponent and M the top two mantissa bits, a Y with
 * -32 <= E < 32 is counted in bins[(E + 32) * 4 + M] — bin i holds [2^e (1 + m / 4), 2^e (1 + (m + 1) / 4)) with e = i / 4 - 32, m = i % 4: four bins an
 * octave over 2^-32 .. 2^32 — and every other Y in one of the five side counters.  No logarithm is taken anywhere, so every counter is an exact integer
 * that a host can restate.  sizeof = 262 * 8. */
typedef struct rmd_luma_histogram {
	uint64_t bins[RMD_LUMA_BINS];
	uint64_t below, above;               /* positive finite Y under 2^-32 (denormals included) / at or over 2^32 */
	uint64_t zero, negative, not_finite; /* Y == +-0 / Y < 0 / NaN or +-inf */
	uint64_t pixels;                     /* all packed pixels = the sum of every counter above */
} rmd_luma_histogram;
/* The luminance histogram of the pixels rmd_resolve_tonemap_tiles would resolve: the same buffers, rects, counts and optional second buffer, and the
 * same rules.  For a packed pixel of rect j and channel c: s_c = accum_dev's sum — plus accum2_dev's, in one rounded addition, when accum2_dev is not
 * NULL —, p_c = s_c / (double)rect_sample_counts[j], and Y = (0.2126 * p_0 + 0.7152 * p_1) + 0.0722 * p_2: each product rounded, then the two additions
 * as bracketed, no fused multiply-add.  A buffer of means (a denoised frame) goes through with counts of 1.  A count of 0 is allowed (zero sums: 0 / 0,
 * counted in not_finite).  Rects may have any size and alignment inside the width x height frame and may overlap (a pixel two rects cover is counted
 * twice); a rect without pixels counts nothing; n_rects = 0 writes an all-zero histogram and returns RMD_OK.  Histograms of disjoint rect lists — several
 * devices, each over its own tiles — add field by field to the histogram of the lists together, exactly and in any order.
 * RMD_ERR_INVALID_ARGUMENT, checked before the device is touched and with the output untouched, in this order: accum_dev NULL, width or height 0, rects or
 * rect_sample_counts NULL with n_rects > 0; accum2_dev overlapping accum_dev; a rect outside the frame; (RMD_ERR_UNSUPPORTED: more than 2^32 - 1 packed
 * pixels;) out_host NULL; and only then a NULL context.  Synchronous; reports an earlier device fault like rmd_resolve_tonemap_tiles.  The cost follows
 * the packed pixels, whatever the number and shape of the rects; the call's device scratch (261 counters and the workgroup table) stays on the context and
 * grows on demand. */
rmd_status rmd_luminance_histogram_tiles(rmd_context *ctx, const double *accum_dev, const double *accum2_dev, uint32_t width, uint32_t height,
                                         const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects, rmd_luma_histogram *out_host);
/* The exposure that puts the histogram's `percentile` of luminance at `target` before gamma: 1 - exp(-Y_p * exposure) = target.  A host function: no
 * context, no device.  N = below + the sum of bins + above (zero, negative and not_finite take no part); N == 0 gives 1.0.  Otherwise
 * r = (uint64_t)ceil(percentile * (double)N) clamped to [1, N]; `below`, bins 0 .. 255 and `above` are accumulated in this order up to the first
 * cumulative count >= r, and Y_p is 2^-32 when that is `below`, the bin's upper edge ldexp(1.0 + (M + 1) * 0.25, E) when it is a bin, 2^32 when it is
 * `above`; *out_exposure = -log1p(-target) / Y_p with the host's libm.  Values to start from: percentile 0.99, target 0.8.
 * RMD_ERR_INVALID_ARGUMENT (text through rmd_last_error(NULL)): h or out_exposure NULL; percentile not finite or outside (0, 1]; target not finite or
 * outside (0, 1). */
rmd_status rmd_exposure_from_histogram(const rmd_luma_histogram *h, double percentile, double target, double *out_exposure);
/*
 * FIREFLY REJECTION from the moments, the stage in front of the filters and of rmd_tile_error (an addition within ABI 6: RMD_ABI_VERSION stays 6, no
 * struct changes, found by its symbol).  A pixel far brighter than all but `rank` of its neighbours — measured in the NEIGHBOUR's standard error,
 * never its own: a firefly's own variance is what hides it from the variance-guided filters — takes a neighbour's sums.
 * S = accum_dev, Q = accum_sq_dev, rects and rect_sample_counts mean what they mean in rmd_denoise: n_i is the count of the rect that covers pixel i, 0 if
 * no rect covers it;
 *     u_ic = S_ic / n_i;   v_ic = max(0, (Q_ic - S_ic*u_ic) / (n_i - 1)) / n_i;   pixel i is VALID if n_i >= 2 and its six sums are finite
 *     Y_i = (0.2126 * u_i0 + 0.7152 * u_i1) + 0.0722 * u_i2           (rmd_luminance_histogram_tiles's luminance)
 *     V_i = (A0 * v_i0 + A1 * v_i1) + A2 * v_i2                       A_c = the binary64 product of the weight with itself
 * every product rounded, the additions as bracketed, nothing fused.
 * The OTHERS of a valid p are the pixels q = p + d with |d_x|, |d_y| <= radius and d != 0 that are inside the frame (not clamped) and valid, ordered by Y
 * descending, ties by the raster order of d (d_y ascending, then d_x ascending).  The DONOR q* is the element at 0-based index `rank`; a p with fewer than
 * rank + 1 others is unchanged.  With
 *     e = (Y_p - ratio * Y_q*) - floor
 * p is a SPIKE if e > 0 and e * e > (k * k) * V_q*.  No square root is taken; a NaN or an infinity in V decides by the IEEE comparisons, so a NaN makes no
 * spike.  Only the donor's variance enters.
 * Output (out_accum_dev = S', out_accum_sq_dev = Q'): a pixel that is not a spike — one that is not valid or that no rect covers included — is a bit copy
 * of its six input values; a spike with n_p == n_q* is a bit copy of the donor's six values; a spike with another count gets
 *     S'_pc = (S_q*c / n_q*) * n_p,   Q'_pc = (Q_q*c / n_q*) * n_p       (the donor's per-sample moments at p's own count)
 * Every decision reads the INPUT only: a replaced pixel is never a donor's stand-in, and nothing cascades.  replaced_host (a HOST array of n_rects words,
 * may be NULL): replaced_host[j] = the number of spikes in rect j, an exact integer.  Both outputs keep the rects' counts: rmd_tile_error, every
 * rmd_denoise*, rmd_resolve_tonemap[_tiles] and rmd_luminance_histogram_tiles take them in place of S and Q unchanged.
 * What the rank means, three consequences:
 *   - `rank` is how many brighter others a pixel may have and still be a spike;
 *   - a run of m bright pixels inside one window survives only if rank < m - 1 (a one-pixel-wide line survives radius 2 with rank 2 — five of it in a
 *     window — and is erased at radius 1 with rank 2);
 *   - the call removes energy, so it is BIASED: the frame's mean goes down by what the spikes held above their donors.
 * RMD_ERR_INVALID_ARGUMENT, all checked before the device is touched, in this order: rmd_denoise's frame and rect rules (width, height > 0; rects and
 * rect_sample_counts non-NULL when n_rects > 0; every rect inside the frame, no two overlapping); 1 <= radius <= 3; rank <= (2 * radius + 1)^2 - 2; k finite
 * and >= 0, ratio finite and >= 1, floor finite and >= 0; the four buffers non-NULL and no two of the four W*H*3-double ranges overlapping; and only then a
 * NULL context.  Synchronous, like rmd_denoise; the call's device scratch (two W*H-word images, the rects and the counters) stays on the context and grows
 * on demand.  Values to start from (not tuned): radius 2, rank 2, k 6, ratio 2, floor 0.
 */
rmd_status rmd_despike(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height,
                       const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects,
                       uint32_t radius, uint32_t rank, double k, double ratio, double floor,
                       double *out_accum_dev, double *out_accum_sq_dev, uint32_t *replaced_host /* n_rects, may be NULL */);
/*
 * FIREFLY REJECTION FOR THE TWO HALVES of a dual-buffer frame, the stage in front of rmd_denoise_dual, its guided, a-trous, region and select forms and
 * rmd_tile_error_dual (an addition within ABI 6: RMD_ABI_VERSION stays 6, no struct changes, found by its symbol).  A firefly is one sample, so it sits in
 * one half only: err = |f_A - f_B| / 2 is large there and wherever the filter smears it, and the cross filter still averages it into the frame.  The call
 * makes exactly the decisions rmd_despike would make on all the samples, and keeps the two halves two independent sample sets.
 * S_A = accum_a_dev, Q_A = accum_sq_a_dev, S_B = accum_b_dev, Q_B = accum_sq_b_dev, rects, rect_counts_a and rect_counts_b mean what they mean in
 * rmd_denoise_dual: n_Ai and n_Bi are the counts of the rect that covers pixel i, 0 if no rect covers it.  Everything is unfused binary64.
 * The MERGED pixel:
 *     n_i = n_Ai + n_Bi;   S_ic = S_Aic + S_Bic;   Q_ic = Q_Aic + Q_Bic      one rounded addition each (rmd_luminance_histogram_tiles's rule for accum2_dev)
 *     pixel i is VALID if n_Ai >= 1, n_Bi >= 1 and its six MERGED sums are finite
 * Finite merged sums imply finite halves; two finite halves whose sum overflows are not valid.  A pixel with an empty half is never a spike and never a
 * donor: the scaled copy below divides by the donor's half count.
 * The decision: u, v, Y, V, the OTHERS of a valid p, their order, the DONOR q* at 0-based index `rank`, e = (Y_p - ratio * Y_q*) - floor and the test
 * e > 0 and e * e > (k * k) * V_q* are rmd_despike's, word for word, on (S, Q, n) with this call's validity.  One decision per pixel serves both halves,
 * and every decision reads the INPUT only.
 * Output (out_accum_a_dev = S'_A, out_accum_sq_a_dev = Q'_A, out_accum_b_dev = S'_B, out_accum_sq_b_dev = Q'_B): a pixel that is not a spike is a bit copy
 * of its twelve input values.  For a spike p with donor q*, each half h on its own:
 *     n_ph == n_q*h:   the six values of half h are bit copies of the donor's half-h values;
 *     otherwise:       S'_phc = (S_q*hc / n_q*h) * n_ph,   Q'_phc = (Q_q*hc / n_q*h) * n_ph
 * A spike takes the donor's HALF sums, never a split of the merged ones: half A of the output holds only half-A samples and stays independent of half B,
 * which the cross filter and err rest on.  The outputs keep the rects' two counts: every dual call takes them in place of the inputs.
 * replaced_host (a HOST array of n_rects words, may be NULL): replaced_host[j] = the number of spikes in rect j, an exact integer.
 * What the definition makes true:
 *   (a) where every rect has both counts >= 1, the spike set and replaced_host equal those of rmd_despike on the buffers S_A + S_B, Q_A + Q_B at n_A + n_B;
 *   (b) where in addition every spike's counts agree with its donor's half by half, S'_A + S'_B and Q'_A + Q'_B (one rounded addition) are rmd_despike's
 *       outputs bit for bit.
 * Bias: the decision is made from the merged sums, so it couples the two halves through the CHOICE of pixels — a selection, not a value: no sample of one
 * half enters the other's sums.  The call removes energy and is BIASED as rmd_despike is.
 * RMD_ERR_INVALID_ARGUMENT, all checked before the device is touched and with the outputs untouched, in this order: rmd_despike's frame and rect rules
 * (width, height > 0; rects, rect_counts_a and rect_counts_b non-NULL when n_rects > 0; every rect inside the frame, no two overlapping); a rect whose two
 * counts add to more than 2^32 - 1; 1 <= radius <= 3; rank <= (2 * radius + 1)^2 - 2; k finite and >= 0, ratio finite and >= 1, floor finite and >= 0; the
 * eight buffers non-NULL and no two of the eight W*H*3-double ranges overlapping; and only then a NULL context.  Synchronous, like rmd_despike, and reports
 * an earlier device fault like it; the call's device scratch (three W*H-word images, the rects, both counts and the counters) stays on the context and grows
 * on demand.  Values to start from (not tuned): rmd_despike's.
 */
rmd_status rmd_despike_dual(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev, const double *accum_sq_b_dev,
                            uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *rect_counts_a, const uint32_t *rect_counts_b,
                            uint32_t n_rects, uint32_t radius, uint32_t rank, double k, double ratio, double floor, double *out_accum_a_dev,
                            double *out_accum_sq_a_dev, double *out_accum_b_dev, double *out_accum_sq_b_dev, uint32_t *replaced_host /* n_rects, may be NULL */);
/*
 * A TILE'S LUMINANCE NOISE, the adaptive check's second measure (an addition within ABI 6: RMD_ABI_VERSION stays 6, no struct or entry point changes,
 * found by its symbol).  rmd_tile_error is a maximum over channels of a maximum over pixels: one dark pixel's one dim channel holds its whole tile.  This
 * call aggregates over the tile and weighs the channels as rmd_luminance_histogram_tiles and the tone-map do.
 * S = accum_dev, Q = accum_sq_dev (W*H*3 doubles each); rect j is reduced on its own at n = rect_counts[j].  Everything is unfused binary64: every product
 * rounded, the additions as bracketed.  Per pixel of rect j, with s and q its six sums:
 *     the pixel is VALID if n >= 2 and its six sums are finite                                              (rmd_despike's rule)
 *     u_c = s_c / n;   v_c = max(0, (q_c - s_c*u_c) / (n - 1)) / n
 *     Y = (0.2126 * u_0 + 0.7152 * u_1) + 0.0722 * u_2                    the luminance of the means
 *     V = (A0 * v_0 + A1 * v_1) + A2 * v_2                                the variance of that luminance's mean; A_c = the weight times itself
 *     d = |Y|; if (!(d > floor)) d = floor;      R = (V / d) / d          two divisions, never V / (d * d); no square root; no input makes R NaN
 * Sum order: the rect's pixels are numbered row-major WITHIN THE RECT, i = 0, 1, ...  Lane t of 256 adds Y, V and R of the valid pixels among
 * i = t, t + 256, t + 512, ... in that order into three running sums that start at +0.0, and counts the valid and the invalid pixels.  The 256 partials of
 * each sum are added exactly as rmd_tile_error_dual adds its partials: within each wave of 64 lanes the lanes 32 apart first, then 16, 8, 4, 2, 1; then
 * the four waves' sums as (w0 + w1) + (w2 + w3).  This gives SY, SV, SR and m = (double)valid.  Then
 *     mean_luma = m ? SY / m : 0;   mean_variance = m ? SV / m : 0;   mean_rel_variance = m ? SR / m : 0
 *     D = |mean_luma|; if (!(D > floor)) D = floor
 *     tile_rms = sqrt(mean_variance) / D;          pixel_rms = sqrt(mean_rel_variance)
 * A rect without pixels gives all zeros.  A rect with pixels and invalid > 0 gives tile_rms = pixel_rms = +inf — its means are still those over the valid
 * pixels —: a tile with a bad pixel never finishes on this rule, as under rmd_tile_error.  A tile_rms or pixel_rms that comes out NaN (inf / inf when the
 * sums overflow) is reported as +inf.  The five fields other than tile_rms and pixel_rms are the same bits on every device and on the host; those two pass
 * through the device's square root.
 * What the two measures mean:
 *   - tile_rms is the RMS standard error of the tile's luminance over the tile's own mean luminance: dark pixels inside a lit tile no longer count for
 *     more than lit ones;
 *   - pixel_rms is the RMS over the tile of each pixel's relative luminance error: a mean instead of a maximum, luminance instead of the worst channel,
 *     but still normalised per pixel.
 * Together with rmd_tile_error they separate the three suspects of an adaptive rule that holds its tiles too long: the maximum, the channel and the
 * normalisation.
 * Rects only have to lie inside the W x H frame; they may overlap or repeat (rmd_tile_error's rule, not the filters').  out_host: a HOST array of n_rects.
 * RMD_ERR_INVALID_ARGUMENT, all checked before the device is touched, in this order: a NULL buffer, width or height 0, or n_rects > 0 with rects, rect_counts
 * or out_host NULL; accum_sq_dev aliasing accum_dev; floor not finite or not > 0; a rect outside the framebuffer; and only then a NULL context.
 * n_rects == 0 is RMD_OK with nothing launched.  Synchronous, like rmd_tile_error; the call's device scratch (rects, counts, results) stays on the context
 * and grows on demand.  One workgroup per rect: made for the adaptive check's tiles, slow for a whole frame passed as one rect.
 */
typedef struct rmd_tile_luma {
	double tile_rms;          /* sqrt(mean_variance) / max(|mean_luma|, floor)                   */
	double pixel_rms;         /* sqrt(mean_rel_variance)                                          */
	double mean_luma;         /* SY / m                                                           */
	double mean_variance;     /* SV / m                                                           */
	double mean_rel_variance; /* SR / m                                                           */
	uint32_t valid, invalid;  /* pixels of the rect that are / are not valid                      */
} rmd_tile_luma;              /* 48 bytes */
rmd_status rmd_tile_luma_error(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height,
                               const rmd_tile_rect *rects, const uint32_t *rect_counts, uint32_t n_rects, double floor, rmd_tile_luma *out_host);
/*
 * A TILE'S VARIANCE WEIGHTED BY LUMINANCE, the adaptive check's measure of the error where the frame is looked at (an addition within ABI 6:
 * RMD_ABI_VERSION stays 6, no struct or entry point changes, found by its symbol).  Every pixel's variance of its luminance's mean is multiplied by a
 * weight that depends on the pixel's luminance alone, and the weight is an entry of a table of RMD_LUMA_WEIGHTS doubles the caller passes — one per
 * counter of rmd_luminance_histogram_tiles, in rmd_luma_histogram's order: the 256 bins, then below, above, zero, negative; not_finite has none.  The
 * device evaluates no transcendental function: a table lookup, one product and the sums.  Any weighting of variance by luminance is such a table:
 * rmd_display_weights makes the squared slope of the library's tone curve (the displayed error, in fractions of the display's full scale: 1/255 is one
 * 8-bit level); all ones is the tile's absolute RMS standard error; 1 / Y^2 per bin approximates rmd_tile_luma_error's pixel_rms.
 * S = accum_dev, Q = accum_sq_dev (W*H*3 doubles each); rect j is reduced on its own at n = rect_counts[j].  Everything is unfused binary64: every product
 * rounded, the additions as bracketed.  Per pixel of rect j, with s and q its six sums:
 *     the pixel is VALID if n >= 2 and its six sums are finite                                              (rmd_despike's rule)
 *     u_c = s_c / n;   v_c = max(0, (q_c - s_c*u_c) / (n - 1)) / n
 *     Y = (0.2126 * u_0 + 0.7152 * u_1) + 0.0722 * u_2                    the luminance of the means
 *     V = (A0 * v_0 + A1 * v_1) + A2 * v_2                                the variance of that luminance's mean; A_c = the weight times itself
 *     k = the counter rmd_luminance_histogram_tiles makes from the 64 bits of Y (E its unbiased exponent, M its top two mantissa bits; -32 <= E < 32:
 *         (E + 32) * 4 + M; positive below 2^-32: 256; at or over 2^32: 257; +-0: 258; Y < 0: 259); a valid pixel whose Y is not finite counts as
 *         INVALID (its sums are finite, so this should not occur)
 *     w = weights[k];   E = (w == 0.0) ? 0.0 : w * V                      one rounded product; V may be +inf, and a zero weight still gives 0
 * Sum order: the rect's pixels are numbered row-major WITHIN THE RECT, i = 0, 1, ...  Lane t of 256 adds Y, V and E of the valid pixels among
 * i = t, t + 256, t + 512, ... in that order into three running sums that start at +0.0, and counts the valid and the invalid pixels.  The 256 partials of
 * each sum are added exactly as rmd_tile_luma_error adds its partials: within each wave of 64 lanes the lanes 32 apart first, then 16, 8, 4, 2, 1; then
 * the four waves' sums as (w0 + w1) + (w2 + w3).  This gives SY, SV, SE and m = (double)valid.  Then
 *     mean_luma = m ? SY / m : 0;   mean_variance = m ? SV / m : 0;   mean_weighted_variance = m ? SE / m : 0
 *     rms = sqrt(mean_weighted_variance)
 * A rect without pixels gives all zeros.  A rect with pixels and invalid > 0 gives rms = +inf — its means are still those over the valid pixels —: a tile
 * with a bad pixel never finishes on this rule, as under rmd_tile_error.  An rms that comes out NaN is reported as +inf.  The five fields other than rms
 * are the same bits on every device and on the host; rms passes through the device's square root.  With all-ones weights mean_luma, mean_variance, valid
 * and invalid are rmd_tile_luma_error's, bit for bit.
 * Rects only have to lie inside the W x H frame; they may overlap or repeat.  weights_host: a HOST array of RMD_LUMA_WEIGHTS; out_host: a HOST array of
 * n_rects.  RMD_ERR_INVALID_ARGUMENT, all checked before the device is touched, in this order: a NULL buffer, width or height 0, or n_rects > 0 with rects,
 * rect_counts, weights_host or out_host NULL; accum_sq_dev aliasing accum_dev; a weight that is NaN, infinite or negative; a rect outside the framebuffer;
 * and only then a NULL context.  n_rects == 0 is RMD_OK with nothing launched.  Synchronous, like rmd_tile_error; the call's device scratch (rects, counts,
 * weights, results) stays on the context and grows on demand; one upload, one launch, one download.  One workgroup per rect: made for the adaptive check's
 * tiles, slow for a whole frame passed as one rect.
 */
#define RMD_LUMA_WEIGHTS 260u   /* the 256 bins, then below, above, zero, negative: luma_bins.hpp's counter order without not_finite */
typedef struct rmd_tile_weighted {
	double rms;                    /* sqrt(mean_weighted_variance) */
	double mean_weighted_variance; /* SE / m */
	double mean_luma;              /* SY / m */
	double mean_variance;          /* SV / m */
	uint32_t valid, invalid;       /* pixels of the rect that are / are not valid */
} rmd_tile_weighted;               /* 40 bytes */
rmd_status rmd_tile_weighted_error(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height,
                                   const rmd_tile_rect *rects, const uint32_t *rect_counts, uint32_t n_rects,
                                   const double *weights_host /* RMD_LUMA_WEIGHTS */, rmd_tile_weighted *out_host);
/* The weights that make rmd_tile_weighted_error measure the DISPLAYED error: per counter the squared slope of the library's own tone curve
 * D(y) = (1 - exp(-y e))^(1/g) at the counter's luminance, e = exposure, g = gamma.  A host function: no context, no device; the host's libm.
 *     t(y) = -expm1(-y * e);   slope(y) = (1/g) * pow(t, 1/g - 1) * e * exp(-y * e);   y_floor = -log1p(-pow(display_floor, g)) / e
 * Bin i, with E = i / 4 - 32 and M = i % 4: y_c = ldexp(1.0 + (M + 0.5) * 0.25, E), the bin's centre, exact; out[i] = slope(max(y_c, y_floor))^2.
 * below, zero and negative take slope(y_floor)^2; above takes slope(2^32)^2, which is 0 at any sane exposure.  Luminances under the one that displays at
 * display_floor take that luminance's slope: D's slope grows without bound towards black for g > 1, and this cap keeps the weight finite (1/255, the first
 * 8-bit level, is the value to start from).  rms is then in fractions of the display's full scale.  The weight is a function of luminance only: it stands
 * for a tone curve applied per channel.
 * Every output is finite and >= 0 for every accepted input: a square that overflows is clamped to the largest finite double (DBL_MAX), and a NaN — inf * 0,
 * when 1/g overflows or pow(display_floor, g) underflows — is written as 0.
 * RMD_ERR_INVALID_ARGUMENT (text through rmd_last_error(NULL)): out_weights NULL; exposure or gamma not finite or not > 0; display_floor not finite or
 * outside (0, 1). */
rmd_status rmd_display_weights(double exposure, double gamma, double display_floor, double *out_weights /* RMD_LUMA_WEIGHTS */);
/*
 * THE DISPLAYED ERROR OF THE FILTERED FRAME, the dual-buffer loop's check by what the viewer sees (an addition within ABI 6: RMD_ABI_VERSION stays 6, no
 * struct or entry point changes, found by its symbol).  rmd_tile_weighted_error weighs the variance of the RAW sums; this call weighs rmd_denoise_dual's
 * per-pixel error estimate of the frame that is DELIVERED, by the luminance of that frame.  out_dev: the filtered means (W*H*3 doubles, any
 * rmd_denoise_dual* or rmd_denoise_atrous_dual* call's out_dev); err_dev: that call's error image (W*H doubles).  The table is rmd_tile_weighted_error's:
 * RMD_LUMA_WEIGHTS doubles, rmd_display_weights' for the displayed error.  Everything is unfused binary64: every product rounded, the additions as
 * bracketed.  Per pixel of rect j, with o_0..2 its three doubles of out_dev and e its double of err_dev:
 *     the pixel is VALID if e is not NaN and o_0, o_1, o_2 are finite.  A pixel that is not dual-valid has err = NaN by rmd_denoise_dual's definition;
 *         e = +inf is valid (h*h overflows at large scales); a negative e is added as it is
 *     Y = (0.2126 * o_0 + 0.7152 * o_1) + 0.0722 * o_2                    rmd_luminance_histogram_tiles's luminance, of the filtered means
 *     k = the counter rmd_luminance_histogram_tiles makes from the 64 bits of Y (rmd_tile_weighted_error states it); a valid pixel whose Y is not
 *         finite (the means are finite, their weighted sum overflowed) counts as INVALID
 *     w = weights[k];   E = (w == 0.0) ? 0.0 : w * e                      one rounded product; e may be +inf, and a zero weight still gives 0
 * Sum order: rmd_tile_weighted_error's, unchanged — the rect's pixels numbered row-major WITHIN THE RECT, lane t of 256 adding Y, e and E of the valid pixels
 * among i = t, t + 256, ... into three sums that start at +0.0 and counting the valid and the invalid pixels; within each wave of 64 the lanes 32 apart
 * first, then 16, 8, 4, 2, 1; then the four waves' sums as (w0 + w1) + (w2 + w3).  This gives SY, SV, SE and m = (double)valid.  Then
 *     mean_luma = m ? SY / m : 0;   mean_variance = m ? SV / m : 0   (the mean of err over the valid pixels);   mean_weighted_variance = m ? SE / m : 0
 *     rms = sqrt(mean_weighted_variance)
 * A rect without pixels gives all zeros.  A rect with pixels and invalid > 0 gives rms = +inf, with the means of the valid pixels.  An rms that comes out
 * NaN (a negative or an inf - inf mean) is reported as +inf.  The means themselves are not guarded: a rect whose err holds negative entries beside +inf, or
 * sums that overflow both ways, has a NaN mean_variance or mean_weighted_variance; with no negative err in the rect — rmd_denoise_dual's err is a mean of
 * squares — every term is >= 0 and no field is NaN.  The five fields other than rms are the same bits on every device and on the host; rms passes
 * through the device's square root.
 * With all-ones weights and a rect without an invalid pixel, rms is rmd_tile_error_dual's result bit for bit on the same device — the same lanes, the same
 * combine, 1.0 * e is exact, m is the pixel count, both take the device's square root — and mean_variance is that result's radicand.
 * What the measure is and is not: err is the mean over the channels of the squared half-difference of the two halves' filtered frames.  As the variance of
 * the LUMINANCE it is exact for a grey difference and an approximation otherwise.  The measure inherits what rmd_denoise_dual says of err: it reads low
 * (it sees variance, not the filter's bias), and it ranks tiles.
 * Rects only have to lie inside the W x H frame; they may overlap or repeat.  weights_host: a HOST array of RMD_LUMA_WEIGHTS; out_host: a HOST array of
 * n_rects.  RMD_ERR_INVALID_ARGUMENT, all checked before the device is touched, in this order: out_dev or err_dev NULL, width or height 0, or n_rects > 0
 * with rects, weights_host or out_host NULL; the ranges of out_dev (W*H*3 doubles) and err_dev (W*H doubles) overlapping; a weight that is NaN, infinite
 * or negative; a rect outside the framebuffer; and only then a NULL context.  n_rects == 0 is RMD_OK with nothing launched.  Synchronous, like
 * rmd_tile_error_dual, and reports an earlier device fault like it; the call's device scratch (rects, weights, results) stays on the context and grows on
 * demand; one upload (rects and weights staged together), one launch, one download.  One workgroup per rect: made for the adaptive check's tiles.
 */
rmd_status rmd_tile_weighted_error_dual(rmd_context *ctx, const double *out_dev /* W*H*3 means */, const double *err_dev /* W*H */,
                                        uint32_t width, uint32_t height, const rmd_tile_rect *rects, uint32_t n_rects,
                                        const double *weights_host /* RMD_LUMA_WEIGHTS */, rmd_tile_weighted *out_host);

/* ---- multi-GPU (no reference counterpart; the reference has no collectives) ---- */
#define RMD_COMM_ID_BYTES 128
/* One process per GPU.  rank 0 calls rmd_comm_unique_id and ships the 128 bytes to the other ranks by any means.
 * Environment: RCCL shares buffers between the ranks through HIP IPC; on hosts whose driver supports dmabuf IPC only, every rank needs
 * HSA_ENABLE_IPC_MODE_LEGACY=0 in its environment BEFORE its first HIP call (the HSA runtime reads its environment once).  The library never
 * changes the environment on its own: a multi-GPU caller either exports the variable or calls rmd_comm_prepare_process() — which sets it to 0
 * unless the environment already holds a value — before rmd_context_create and any other HIP call of the process; single-GPU callers are not
 * affected.  rmd_comm_create names the variable in its error text when RCCL's initialisation fails without it. */
rmd_status rmd_comm_prepare_process(void);
rmd_status rmd_comm_unique_id(uint8_t id_out[RMD_COMM_ID_BYTES]);
rmd_status rmd_comm_create(rmd_context *ctx, const uint8_t id[RMD_COMM_ID_BYTES], int32_t rank, int32_t world_size,
                           rmd_comm **out);
void rmd_comm_destroy(rmd_comm *comm);
/* In-place ncclReduce(sum, f64) of the accumulated framebuffer to `root` over xGMI.
 * Every pixel is non-zero on exactly one rank, so the sum is bit-identical to a 1-GPU render. */
rmd_status rmd_reduce_framebuffer(rmd_comm *comm, double *accum_dev, size_t n_doubles, int32_t root);
/* Same, enqueue only (on the context's stream, behind the renders enqueued before it); pair with rmd_context_synchronize.  Lets a rank queue
 * zeroing, rmd_render_tiles_async and the reduce of several frames back to back. */
rmd_status rmd_reduce_framebuffer_async(rmd_comm *comm, double *accum_dev, size_t n_doubles, int32_t root);

/* ---- host-side grid build (AccGrid::build_from_mesh, core/src/geometry/acc_grid.rs:6-83) ---- */
typedef struct rmd_grid_build rmd_grid_build; /* owns the arrays a rmd_grid_desc points at */
/* tri_pos/tri_nrm: n_tris*9 doubles each (host).  Computes mesh bounds (mesh.rs:123-140), resolution,
 * cell_size, cells, mapping_table.  RMD_ERR_GRID_INDEX where the reference would panic: the
 * `x + res.x*(y + z*res.z)` index (acc_grid.rs:61) running past the cell array, a cell bound that does not fit usize (:44-51: a
 * triangle of NaNs), a zero resolution (:54: an infinite vertex, a volume that overflows or underflows).
 * The bounds are folded over the vertices in order from the reference's seeds; a NaN coordinate is skipped, and where a bound is
 * zero — the reference leaves the sign of a +0.0 / -0.0 tie to the platform's f64::min / max — the LATER vertex's zero is the bound. */
rmd_status rmd_grid_build_from_mesh(const double *tri_pos, const double *tri_nrm, uint64_t n_tris,
                                    rmd_grid_build **out);
/* The same build on the GPU of `ctx` (bounds and resolution on the host as above; per-cell atomic counts, device scan, fill and
 * per-cell sort on the device).  Status for status, and bounds (with the signs of their zeros), resolution, cell size and both tables byte
 * for byte, what rmd_grid_build_from_mesh gives (tests/test_gpu_grid_build.py).  The per-cell sort is an insertion sort in one lane,
 * quadratic in the length of a cell's run: a mesh with tens of thousands of triangles in ONE cell is better built on the host. */
rmd_status rmd_grid_build_from_mesh_gpu(rmd_context *ctx, const double *tri_pos, const double *tri_nrm, uint64_t n_tris,
                                        rmd_grid_build **out);
/* Fills `desc` with pointers into `build` (valid until rmd_grid_build_destroy). */
rmd_status rmd_grid_build_describe(const rmd_grid_build *build, rmd_grid_desc *desc);
void rmd_grid_build_destroy(rmd_grid_build *build);

#ifdef __cplusplus
}
#endif
#endif /* RAYMOND_HIP_H */
