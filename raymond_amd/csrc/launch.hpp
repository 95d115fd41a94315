// Host-callable launchers of kernels.hip (internal to the library).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/raymond_hip.h"
#include "denoise_host.hpp"
#include "device_types.hpp"

// entries per lane in the list-mode path record: one per trace() depth, bounce_limit <= 16
#define RMD_PATH_STRIDE 17
// include/raymond_hip.h: RMD_MAX_BOUNCE_LIMIT (api.cpp asserts the two agree) — a path has at most this many segments, which bounds the render loops
#define RMD_MAX_BOUNCE_LIMIT_DEV 16u

namespace rmd {

enum ProbeOp {
	PROBE_PHILOX = 0,
	PROBE_UNIFORM,
	PROBE_SPHERE_INTERSECT,
	PROBE_SPHERE_NORMAL,
	PROBE_PLANE_INTERSECT,
	PROBE_AABB_INTERSECT,
	PROBE_TRIANGLE_INTERSECT,
	PROBE_TRIANGLE_NORMAL,
	PROBE_ONB,
	PROBE_COSINE_HEMISPHERE,
	PROBE_SAMPLE_GGX,
	PROBE_GGX_DISTRIBUTION,
	PROBE_GEOMETRY_SMITH,
	PROBE_FRESNEL_SCHLICK,
	PROBE_PRIMARY_RAY,
	PROBE_ELEMENTARY,
	PROBE_PRETEST_PAIR,
	PROBE_OP_COUNT
};

// LDS a workgroup may use: the CU's 160 KiB less a margin for alignment
constexpr size_t kLdsBudgetBytes = 160u * 1024u;
// LDS bytes reserved for the grids' occupancy masks (shared by the waves of a workgroup)
constexpr size_t kMaskBudgetBytes = 48u * 1024u;
// doubles per entry of the per-sample scratch of split launches: r, g, b and one of padding = one 32-byte sector
constexpr uint32_t kSampleStride = 4;
// walk batching (kernels.hip): lanes of a wave that must be waiting for a grid walk before one is run
constexpr uint32_t kWalkBatchDefault = 32;
// fewest samples per pixel a work item of a split launch of a grid scene may hold (api.cpp: choose_split; RMD_TUNE_SPLIT_MIN_SAMPLES overrides)
constexpr uint32_t kSplitMinSamplesGrid = 4;
// scenes without grids: fewest samples per pixel a launch that is too short to split runs as ONE buffered item per wave tile (role-sorted trips)
// instead of in direct mode (api.cpp: choose_split)
constexpr uint32_t kSortedMinSamples = 128;
// split launches of scenes with grids of at most this many samples per pixel run the instantiation whose waves chain their work items: all of
// them since the round's second half (the chained instantiation used to spill 27 registers against 15 and lost 2.6 % at 500 samples per pixel —
// hence a limit of 96 —; at 11 against 9 it wins at every size: C3 at 128 / 200 / 500 spp 101.7 / 157.2 / 387.8 -> 98.9 / 154.1 / 384.5 ms)
constexpr uint32_t kChainMaxSamples = 0x7FFFFFFF;
// walks put aside (grid_walk.hpp: cut_lanes): a walk call leaves its last K walkers to the wave's next call
constexpr uint32_t kWalkCutDefault = 7; // (round 6: 4 -> 7 — the queued form's walks have 60 rays: C3 at 200 spp 120.1 -> 118.9 ms; the lane-per-path form times within 1 % for 2 .. 12)
// largest |roughness| a material may have: keeps the GGX sampling angle below 2^45 (device_core.hpp, sincos_cw)
constexpr double kMaxRoughness = 512.0;
// smallest non-zero |roughness|: the specular weight's denominator holds (roughness^2 / 8)^2 (device_core.hpp: next_ray), which must not underflow
constexpr double kMinRoughness = 1e-12;
// waves per workgroup of the grid instantiation (they share the LDS occupancy masks)
// 4-wave workgroups: 4 of them (16 waves) fit a CU's LDS beside their staged masks and retire at a finer grain than 8-wave ones
constexpr uint32_t kGridWavesPerWg = 4;
// waves of a persistent workgroup (one per CU: all 16 wave slots that 128 registers per lane leave)
constexpr uint32_t kPersistWavesPerWg = 16;
constexpr uint32_t kGridPersistWavesPerWg = 16; // ... of the grid instantiation
// the spheres kernel's split launches (render_kernel.hpp: render_wave_sorted): entries of a wave's two hit stacks together and waves of a
// persistent workgroup — 16 areas of 168 entries (60 bytes each: an entry holds no normal) and the object table fit the CU's 160 KB
constexpr uint32_t kSortSlots = 168;
constexpr uint32_t kSortedWavesPerWg = 16; // waves of one persistent workgroup (one per CU)
constexpr size_t kSortPoolBytes = 60u * kSortSlots; // per-wave LDS (sizeof(HitStack): 6 doubles + 3 words an entry)
// every wave's LDS area ends with 16 bytes of bookkeeping (render_kernel.hpp: word 0 = 1 + the work item a persistent wave drew last)
constexpr size_t kWaveHeadBytes = 16u;
// the form a render launch was made in (render_kernel.hpp: launch_render) -> rmd_launch_info
struct LaunchShape {
	uint32_t persistent = 0, waves_per_wg = 0, queued = 0, resident_waves = 0, chained = 0;
};
// The form of one render launch, decided on the host from the scene's LDS alone (render_kernel.hpp: plan_launch): which instantiation —
// render_kernel<MODE, GRID, persistent, chained, queued> or render_kernel_moments<MODE, GRID, persistent> —, its waves per workgroup, the per-wave
// area it is charged, its dynamic LDS and its workgroups.  launch_render launches exactly this; tests/test_launch_plan.py checks it over every
// scene check_render_args admits (rmd_probe_launch_plan).
struct LaunchPlan {
	uint32_t persistent = 0, queued = 0, chained = 0, moments = 0, waves_per_wg = 0, workgroups = 0;
	size_t wave_lds = 0, lds = 0;
};
// mode: render_kernel.hpp's kModeTiles / kModeTilesBuffered / kModeList.  queues: path queues are attached (P.queue_buf); persist: the persistent
// form was asked for (n_cus and P.work_counter); chain_items: P.chain_items; moments: the squares are asked for (out_sq)
LaunchPlan plan_render_launch(int mode, bool grid, uint32_t n_objects, uint32_t mask_words_total, bool queues, bool persist, bool chain_items, bool moments,
                              uint32_t n_waves, uint32_t n_cus);
// the sizes the plan is made of, for instantiation (mode, grid): out[0] the LDS budget, [1] sizeof(DevObject), [2] the per-wave area of the
// instantiation's unqueued kernels, [3] the queued form's, [4] waves of its persistent workgroup, [5] kGridWavesPerWg, [6] kSortPoolBytes,
// [7] kMaskBudgetBytes
void render_lds_sizes(int mode, bool grid, uint64_t out[8]);
// paths a wave of the queued form may have in flight (render_kernel.hpp: render_wave_queued; at least 192, a multiple of 64)
constexpr uint32_t kQueuePaths = 256;
inline size_t path_queue_bytes_host(uint32_t cap) { return (size_t)cap * (9u * 8u + 13u * 8u + 4u * 4u + 9u * 4u); } // (render_kernel.hpp: path_queue_bytes)
static_assert(kQueuePaths >= 192u && kQueuePaths % 64u == 0u, "two stacks short of a full trip + the 64 paths of a generation trip");
size_t render_lds_bytes(uint32_t n_objects, uint32_t mask_words_total, uint32_t waves_per_wg);
// n_cus > 0 and P.work_counter set: grid scenes run as persistent workgroups (render_kernel.hpp).  accum_sq (optional): every sample's square is
// added there too, in the same order (rmd_render_tiles_moments)
hipError_t launch_render_tiles(hipStream_t stream, const RenderParams &P, const DevObject *objs, const DevGrid *grids,
                               const WaveTile *wave_tiles, double *accum, uint32_t n_cus = 0, LaunchShape *shape = nullptr, double *accum_sq = nullptr);
// out[i] = the relative standard error of rect i's worst pixel and channel (kernels.hip: tile_error_kernel; rects and out are device memory)
hipError_t launch_tile_error(hipStream_t stream, const double *accum, const double *accum_sq, const rmd_tile_rect *rects, uint32_t n_rects, uint32_t W,
                             uint32_t sample_count, double floor, double *out);
// rmd_denoise (denoise.hip): output tile height (the width is 32 or 24: denoise_tile_width), eps of the distance, the argument limits
constexpr uint32_t kDenoiseTile = 16;
constexpr double kDenoiseEps = 1e-10;
constexpr uint32_t kDenoiseMaxRadius = 12, kDenoiseMaxPatch = 4;
constexpr uint32_t kDenoiseMaxCandidates = (uint32_t)RMD_DENOISE_MAX_CANDIDATES, kDenoiseMaxSelectWindow = 5; // rmd_denoise_dual_select
constexpr int kDenoiseFeat = (int)RMD_FEATURE_CHANNELS; // rmd_denoise_guided: feature channels per pixel
// dynamic LDS of denoise_kernel<tile_width>: the apron's u and v (48 B a pixel) and the term image with its row sums
size_t denoise_lds_bytes(uint32_t tile_width, uint32_t radius, uint32_t patch_radius);
// 32 when that tile's LDS fits the budget (every (r, f) but r = 12 with f = 4: 168,192 B), else 24 (145,152 B there)
uint32_t denoise_tile_width(uint32_t radius, uint32_t patch_radius);
// What every denoise launcher is given of the frame (host-only plain structs: no kernel takes one).  The W x H frame's sums — accum_a / accum_sq_a alone for
// the single-buffer filters, both halves for the dual ones —, the features (W*H*7 doubles each, pixel-interleaved; both null: no feature weight, and then
// counts_f, k_f, tau and the features' scratch are not read), and in device memory the rects with their counts: rect i holds counts_a[i] and counts_b[i]
// samples and counts_f[i] feature samples.  count_image_columns: the workgroups given to each rect when the per-pixel counts are painted
struct DenoiseInput {
	const double *accum_a, *accum_sq_a, *accum_b, *accum_sq_b, *feat, *feat_sq;
	const rmd_tile_rect *rects;
	const uint32_t *counts_a, *counts_b, *counts_f;
	uint32_t n_rects, count_image_columns, W, H;
};
// checked by the caller (api_denoise.cpp); k_f, tau and slope are read only with features.  slope (the _slope calls; 0 everywhere else): at 0 every
// launcher launches and reads exactly what it did without it
struct DenoiseWeights {
	double k, alpha, k_f, tau;
	double slope = 0.0;
};
// The slope floors (denoise.hip: feature_slope_kernel): slope_planes = the seven planes m_j = (slope * slope) * (h_j + v_j), W*H doubles each, from the 14
// planes feat_planes that launch_denoise_planes / launch_dual_planes have made on the same stream.  Always the whole frame (the non-local-means launchers and
// the whole-frame a-trous ones call it; rmd_denoise_atrous_dual_slope_region makes its floors over its own block table)
hipError_t launch_feature_slope(hipStream_t stream, const double *feat_planes, uint32_t W, uint32_t H, double slope, double *slope_planes);
// rmd_denoise / rmd_denoise_guided[_slope] (denoise.hip): out = the denoised means.  Scratch: n_img W*H uint32 for the per-pixel counts; with features
// feat_planes, 14 * W*H doubles for the planar per-pixel f and g; with features and w.slope > 0 slope_planes, 7 * W*H doubles (else not read, may be null)
hipError_t launch_denoise_guided(hipStream_t stream, const DenoiseInput &in, const DenoiseWeights &w, uint32_t radius, uint32_t patch_radius, uint32_t *n_img,
                                 double *feat_planes, double *slope_planes, double *out);
// The preamble of launch_denoise_guided on its own (denoise.hip), for the filters of other units: n_img = the per-pixel counts, and when feat / feat_sq
// are given feat_planes = the 14 planar images of the per-pixel f and g (a pixel that is not feature-valid keeps a NaN in plane 0)
hipError_t launch_denoise_planes(hipStream_t stream, const DenoiseInput &in, uint32_t *n_img, double *feat_planes);
// rmd_denoise_atrous (denoise_atrous.hip): out = the frame after `levels` levels of the edge-avoiding a-trous filter (levels = 0: S / n).  n_img and
// feat_planes as launch_denoise_guided's; cv is 12 * W*H doubles of scratch, the two sets of six planes (c and v) the levels alternate between.  levels is
// checked by the caller.  With features, levels > 0 and w.slope > 0 (rmd_denoise_atrous_slope): slope_planes is 7 * W*H doubles more, made once by
// launch_feature_slope and read by every level; else it is not read and may be null
constexpr uint32_t kAtrousMaxLevels = (uint32_t)RMD_ATROUS_MAX_LEVELS;
hipError_t launch_denoise_atrous(hipStream_t stream, const DenoiseInput &in, const DenoiseWeights &w, uint32_t levels, uint32_t *n_img, double *cv, double *feat_planes,
                                 double *slope_planes, double *out);
// rmd_denoise_dual (denoise_dual.hip): out = the cross-filtered means of the two halves, err (may be null) the per-pixel error estimate, W*H doubles.
// Scratch: n_img 2 * W*H uint32, planes 12 * W*H doubles, f_b 3 * W*H doubles; the tile shape and LDS are denoise_kernel's.  table null: every pixel
// of out and err is written.  table not null (rmd_denoise_dual_region; device memory): n_blocks entries (x0, y0, x_end, y_end), one per workgroup of
// denoise_tile_width(radius, patch_radius) x 16 pixels at (x0, y0); only the pixels before (x_end, y_end), inside the frame, are written.
// With features (rmd_denoise_dual_guided[_region]): n_f_img is W*H uint32 and feat_planes 14 * W*H doubles of further scratch.  Without: exactly the
// launches made without the feature.  With features and w.slope > 0 (the _slope calls): slope_planes is 7 * W*H doubles more, made over the whole frame in
// the region form too; else it is not read and may be null
hipError_t launch_denoise_dual(hipStream_t stream, const DenoiseInput &in, const DenoiseWeights &w, uint32_t radius, uint32_t patch_radius, uint32_t *n_img, double *planes,
                               double *f_b, uint32_t *n_f_img, double *feat_planes, double *slope_planes, const DualBlock *table, uint32_t n_blocks, double *out,
                               double *err);
// What every dual call makes first, once (denoise_dual.hip; also for the filters of other units): n_img = both halves' per-pixel counts (2 * W*H uint32),
// planes = the twelve planar u / v images (half h's u in planes 6h + c, its v in 6h + 3 + c; a pixel that is not dual-valid keeps a NaN in plane 0), and
// with features n_f_img and feat_planes = their per-pixel counts and their 14 planar f and g at that count (which read the dual-validity mark just left)
hipError_t launch_dual_planes(hipStream_t stream, const DenoiseInput &in, uint32_t *n_img, double *planes, uint32_t *n_f_img, double *feat_planes);
// rmd_denoise_atrous_dual (denoise_atrous_dual.hip): out / err (err may be null) = rmd_denoise_dual's combination of the two halves after `levels`
// levels of the a-trous filter, each half under the other's weights.  n_img, n_f_img and feat_planes as launch_denoise_dual's; state is 24 * W*H doubles of
// scratch, the two sets of twelve planes the levels alternate between.  levels is checked by the caller.  slope_planes as launch_denoise_atrous's
// (rmd_denoise_atrous_dual_slope): one set of floors for every level and both halves
hipError_t launch_denoise_atrous_dual(hipStream_t stream, const DenoiseInput &in, const DenoiseWeights &w, uint32_t levels, uint32_t *n_img, double *state,
                                      uint32_t *n_f_img, double *feat_planes, double *slope_planes, double *out, double *err);
// rmd_denoise_atrous_dual_region (denoise_atrous_dual.hip): launch_denoise_atrous_dual for the pixels of a region, through levels + 1 block tables of
// 64 x 4-pixel workgroups (entries table_first[i] .. + table_count[i] of `table`, device memory; the two index arrays are host memory): table 0 the
// prologue's — the pixels whose planes are made —, table 1 + l level l's; the last level's (table 0 at levels = 0) is cut from the region's rects and
// carries their far corners, so only the region's pixels of out and err are written.  Every table has at least one entry.  n_img, state, n_f_img and
// feat_planes as launch_denoise_atrous_dual's; what they hold outside the tables' pixels is not defined.  slope_planes (rmd_denoise_atrous_dual_slope_region at
// slope > 0, else not read): 7 * W*H doubles, made on table 1's pixels only — level 0's, which hold every later level's — from the f planes of table 0
hipError_t launch_denoise_atrous_dual_region(hipStream_t stream, const DenoiseInput &in, const DenoiseWeights &w, uint32_t levels, uint32_t *n_img, double *state,
                                             uint32_t *n_f_img, double *feat_planes, double *slope_planes, const DualBlock *table, const uint32_t *table_first,
                                             const uint32_t *table_count, double *out, double *err);
// rmd_denoise_dual_select (denoise_dual.hip): launch_dual_planes once, then per candidate (a HOST array, checked by the caller) its two cross passes with
// their gain images and its SURE image, then the winners and the blend.  Scratch: n_img and planes as above; cand_img 7 * W*H doubles per candidate
// (f_A 3, f_B 3, SURE 1); gain 2 * W*H doubles (g_A, g_B, reused by every candidate); win_img W*H uint32; n_f_img and feat_planes as above, read only when
// a candidate is guided.  err, sure and win (W*H each) may be null.  cand_slopes (rmd_denoise_dual_select_slope; a HOST array of n_cands, or null = all 0):
// a guided candidate's slope; slope_planes, 7 * W*H doubles, is one set for all of them, remade whenever the next guided candidate's slope > 0 differs from
// the one it holds, and not read (may be null) when none is > 0
hipError_t launch_denoise_dual_select(hipStream_t stream, const DenoiseInput &in, uint32_t radius, uint32_t patch_radius, const rmd_denoise_candidate *cands,
                                      const double *cand_slopes, uint32_t n_cands, uint32_t sure_window, uint32_t select_window, uint32_t *n_img, double *planes,
                                      double *cand_img, double *gain, uint32_t *win_img, uint32_t *n_f_img, double *feat_planes, double *slope_planes, double *out,
                                      double *err, double *sure, uint32_t *win);
// out[i] = sqrt(the mean of err over rect i's pixels), +inf if one of them is NaN (denoise_dual.hip: tile_error_dual_kernel; rects and out are device memory)
hipError_t launch_tile_error_dual(hipStream_t stream, const double *err, const rmd_tile_rect *rects, uint32_t n_rects, uint32_t W, double *out);
// rmd_render_features (features.hip): for each of the P.n_work wave tiles, the first-hit features of samples P.sample_begin .. + P.sample_count - 1
// added to feat (and their squares to feat_sq when it is not null), W*H*RMD_FEATURE_CHANNELS doubles each
hipError_t launch_features(hipStream_t stream, const RenderParams &P, const DevObject *objs, const DevGrid *grids, const WaveTile *wave_tiles, double *feat,
                           double *feat_sq);
// rmd_render_ids (ids.hip): for each of the P.n_work wave tiles, the first-hit keys of samples P.sample_begin .. + P.sample_count - 1 entered into the
// pixels' records of `ids`, W*H*RMD_ID_WORDS words (ids_rule.hpp: ids_insert)
hipError_t launch_ids(hipStream_t stream, const RenderParams &P, const DevObject *objs, const DevGrid *grids, const WaveTile *wave_tiles, uint32_t *ids);
// rmd_ids_matte (ids.hip): matte[i] = pixel i's matte over the n_keys ascending, distinct keys (ids_rule.hpp: ids_matte_pixel; device memory, at most 2048),
// and *other_pixels (zeroed by the caller) += the pixels whose record has other != 0
hipError_t launch_ids_matte(hipStream_t stream, const uint32_t *ids, uint64_t n_pixels, const uint32_t *keys, uint32_t n_keys, double *matte, unsigned long long *other_pixels);
// rmd_render_ao (ao.hip): for each of the P.n_work wave tiles, samples P.sample_begin .. + P.sample_count - 1 counted into the pixels' records of `ao`,
// W*H*RMD_AO_WORDS words (ao_rule.hpp: ao_count): occluded where the diffuse bounce ray off the first hit meets an object nearer than max_distance
hipError_t launch_ao(hipStream_t stream, const RenderParams &P, const DevObject *objs, const DevGrid *grids, const WaveTile *wave_tiles, uint32_t *ao, double max_distance);
// rmd_ao_resolve (ao.hip): out[i] = pixel i's open / (open + occluded), empty_value where the sum is 0 (ao_rule.hpp: ao_resolve_pixel), and
// *empty_pixels (zeroed by the caller) += the pixels where it is
hipError_t launch_ao_resolve(hipStream_t stream, const uint32_t *ao, uint64_t n_pixels, double empty_value, double *out, unsigned long long *empty_pixels);
// rmd_intersect_rays (rays.hip): hits[i] = Scene::intersect on ray i with rmd_render_features' normal, i < n_rays <= RMD_MAX_RAYS; of P the scene's fields
// are read (n_objects, n_grids, mask_words_total, axis_pairs, visit_mask).  n_cus sizes the launch (rays_plan.hpp)
hipError_t launch_rays(hipStream_t stream, const RenderParams &P, const DevObject *objs, const DevGrid *grids, uint32_t n_cus, const double *rays, uint64_t n_rays,
                       rmd_ray_hit *hits);
// the launch that would be (rays.hip): the plan, the workgroup's dynamic LDS and its per-wave area (both may be null); false: the scene's tables do not fit
struct RaysPlan;
bool plan_rays_launch(const RenderParams &P, uint64_t n_rays, uint32_t n_cus, RaysPlan &plan, size_t *lds, size_t *wave_lds);
// rmd_camera_rays (rays.hip): rays[6i ..] = the pinhole primary ray of pixel xy[2i], xy[2i + 1] at uv[2i], uv[2i + 1] (uv null: 0.5, 0.5); device memory
hipError_t launch_camera_rays(hipStream_t stream, const RenderParams &P, const uint32_t *xy, const double *uv, uint64_t n_rays, double *rays);
hipError_t launch_render_list(hipStream_t stream, const RenderParams &P, const DevObject *objs, const DevGrid *grids,
                              const ListWork *list, double *rgb_out, int32_t *path_obj, uint32_t *path_sub);
// tile rectangles of a frame <-> a packed buffer (kernels.hip: tile_copy_kernel); `first[i]` = pixels in front of rect i
hipError_t launch_tile_copy(hipStream_t stream, bool to_packed, double *frame, double *packed, const rmd_tile_rect *rects, const uint64_t *first,
                            uint32_t n_rects, uint32_t W);
// pixel += the per-sample radiance of a split launch, in sample order (kernels.hip: sum_kernel)
hipError_t launch_sum(hipStream_t stream, const RenderParams &P, const WaveTile *wave_tiles, double *accum);
// |255 * tm - k| below this flags a pixel for the host's libm (kernels.hip: tonemap_kernel); device exp / pow are good to ~1e-12 there
constexpr double kTonemapGuard = 1e-7;
hipError_t launch_tonemap(hipStream_t stream, const double *accum, uint8_t *rgb8, size_t n_pixels, double sample_count,
                          double exposure, double inv_gamma, uint32_t *flagged, uint32_t *n_flagged);
// rmd_resolve_tonemap_tiles (resolve_tiles.hip): one workgroup per run of the table (resolve_tiles_host.hpp; device memory); rgb8: 3 bytes per packed
// pixel, padded to 4, at a 4-byte boundary; flagged: one word per packed pixel, n_flagged: one zeroed word; accum2 may be null
struct ResolveRun;
hipError_t launch_resolve_tiles(hipStream_t stream, const double *accum, const double *accum2, uint32_t W, const ResolveRun *runs, uint32_t n_runs,
                                double exposure, double inv_gamma, uint8_t *rgb8, uint32_t *flagged, uint32_t *n_flagged);
// rmd_luminance_histogram_tiles (luma_histogram.hip): one workgroup per run of the same table; counters: luma_bins.hpp's kLumaCounters uint64, zeroed by
// the caller, to which the workgroups add; accum2 may be null
hipError_t launch_luma_histogram(hipStream_t stream, const double *accum, const double *accum2, uint32_t W, const ResolveRun *runs, uint32_t n_runs,
                                 uint64_t *counters);
// rmd_despike (despike.hip): out_accum / out_accum_sq = the frame's sums with every spike replaced by its donor (despike_rule.hpp has the rule); only
// in.accum_a / in.accum_sq_a, the rects and counts_a are read.  Scratch: n_img W*H uint32 for the per-pixel counts, rect_img W*H uint32 for the per-pixel
// rect index, `replaced` in.n_rects uint32 to which the workgroups add each rect's spikes (zeroed here).  replaced null: nothing is counted and rect_img is
// not read (may be null).  radius is 1 .. 3; the other arguments are checked by the caller
hipError_t launch_despike(hipStream_t stream, const DenoiseInput &in, uint32_t radius, uint32_t rank, double k, double ratio, double floor, uint32_t *n_img,
                          uint32_t *rect_img, double *out_accum, double *out_accum_sq, uint32_t *replaced);
// launch_despike's counting preamble on its own (despike.hip), for rmd_despike_dual: `replaced` (in.n_rects words, n_rects > 0) zeroed and rect_img painted
// with each covered pixel's rect index
hipError_t launch_rect_index_image(hipStream_t stream, const DenoiseInput &in, uint32_t *rect_img, uint32_t *replaced);
// rmd_despike_dual (despike_dual.hip): the four outputs = the two halves' sums with every spike of the MERGED pixel replaced half by half from its donor
// (despike_dual_rule.hpp over despike_rule.hpp has the rule).  in's four sum buffers, the rects, counts_a and counts_b are read.  Scratch: n_img 2 * W*H
// uint32 — half A's per-pixel counts, then half B's, each painted by launch_denoise_planes —, rect_img and `replaced` as launch_despike's.  radius is
// 1 .. 3; the other arguments, and that no rect's two counts add past 2^32 - 1, are checked by the caller
hipError_t launch_despike_dual(hipStream_t stream, const DenoiseInput &in, uint32_t radius, uint32_t rank, double k, double ratio, double floor, uint32_t *n_img,
                               uint32_t *rect_img, double *out_accum_a, double *out_accum_sq_a, double *out_accum_b, double *out_accum_sq_b, uint32_t *replaced);
// rmd_tile_luma_error (tile_luma.hip): out[i] = rect i's result (tile_luma_rule.hpp: TileLuma, rmd_tile_luma's layout) from in.accum_a / in.accum_sq_a at
// in.counts_a[i], one workgroup per rect; the rects, the counts and `out` are device memory.  Nothing else of `in` is read.  floor is checked by the caller
struct TileLuma;
hipError_t launch_tile_luma(hipStream_t stream, const DenoiseInput &in, double floor, TileLuma *out);
// rmd_tile_weighted_error (tile_weighted.hip): out[i] = rect i's result (tile_weighted_rule.hpp: TileWeighted, rmd_tile_weighted's layout) from in.accum_a /
// in.accum_sq_a at in.counts_a[i], one workgroup per rect; the rects, the counts, the RMD_LUMA_WEIGHTS `weights` and `out` are device memory.  Nothing else
// of `in` is read.  The weights are checked by the caller
struct TileWeighted;
hipError_t launch_tile_weighted(hipStream_t stream, const DenoiseInput &in, const double *weights, TileWeighted *out);
// rmd_tile_weighted_error_dual (tile_weighted_dual.hip): out[i] = rect i's result (rmd_tile_weighted's layout) from the filtered frame `out_img` (3 doubles a
// pixel) and the error image `err` (one), rows W pixels apart, one workgroup per rect; the rects, the RMD_LUMA_WEIGHTS `weights` and `out` are device
// memory.  The rects and the weights are checked by the caller
hipError_t launch_tile_weighted_dual(hipStream_t stream, const double *out_img, const double *err, const rmd_tile_rect *rects, uint32_t n_rects, uint32_t W,
                                     const double *weights, TileWeighted *out);
hipError_t launch_probe(hipStream_t stream, int op, uint32_t n, const double *in, int in_stride, double *out, int out_stride,
                        const RenderParams &P);
hipError_t launch_probe_scene(hipStream_t stream, int mode, uint32_t g, uint32_t n, const DevObject *objs, uint32_t n_objects,
                              const DevGrid *grids, uint32_t n_grids, uint32_t mask_words_total, uint32_t axis_pairs, const double *rays, double *out);
// the DEEP walk on grid `g`, one wave per `rays_per_wave` rays (probe_kernels.hip: probe_grid_deep_kernel); *stuck is raised by a wave that reaches its call bound
hipError_t launch_probe_grid_deep(hipStream_t stream, uint32_t g, uint32_t n, const DevGrid *grids, uint32_t n_grids, uint32_t mask_words_total, const double *rays,
                                  uint32_t cut_lanes, uint32_t cut_round, uint32_t rays_per_wave, uint32_t walk_steps_bound, double *out, uint32_t *stuck);

} // namespace rmd
