/*
 * raymond_hip_probe.h — diagnostic entry points, in libraymond_hip_probe.so (a separate library that links against
 * libraymond_hip.so and takes its rmd_context / rmd_scene handles; the product library exports none of these).
 *
 * Each probe runs ONE device function of the hot path on the GPU over a batch of host-supplied
 * inputs, so the parity tests can compare it with the CPU oracle function by function
 * (known-answer level of the test pyramid).  They are not part of the drop-in boundary; a host
 * renderer never calls them.  All pointers are HOST pointers; the library stages them through HBM.
 * Argument layouts match the oracle's batched functions (oracle/oracle.h): rays are 6 doubles
 * (origin xyz, direction xyz); hit[i] is 1/0 and t[i] is meaningful only where hit[i] = 1.
 * Each cites the reference function whose device implementation it exercises.
 */
#ifndef RAYMOND_HIP_PROBE_H
#define RAYMOND_HIP_PROBE_H

#include "raymond_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* RNG (replaces rand::random::<f64>(), src/trace.rs:260 etc.) */
rmd_status rmd_probe_philox4x32_10(rmd_context *ctx, size_t n, const uint32_t *ctr4, const uint32_t *key2, uint32_t *out4);
/* per entry 5 doubles: the two 53-bit uniforms and the 22-bit uniform of Philox block `block` of (pixel, sample) as the jitter /
 * lens draws take them (next2), then (r, r1, r2) as a shaded depth takes them (next3) — include/raymond_hip.h "RNG" */
rmd_status rmd_probe_block_uniforms(rmd_context *ctx, uint64_t seed, size_t n, const uint32_t *pixel, const uint32_t *sample,
                                    const uint32_t *block, double *out5);
/* core/src/geometry/primitives/sphere.rs:11-27, :31-35 */
rmd_status rmd_probe_sphere_intersect(rmd_context *ctx, size_t n, const double *sphere4, const double *ray6, int32_t *hit, double *t);
rmd_status rmd_probe_sphere_normal(rmd_context *ctx, size_t n, const double *sphere4, const double *ray6, const double *t, double *n3);
/* core/src/geometry/primitives/plane.rs:11-24 */
rmd_status rmd_probe_plane_intersect(rmd_context *ctx, size_t n, const double *plane6, const double *ray6, int32_t *hit, double *t);
/* core/src/geometry/primitives/aabb.rs:10-31 */
rmd_status rmd_probe_aabb_intersect(rmd_context *ctx, size_t n, const double *aabb6, const double *ray6, int32_t *hit, double *t);
/* core/src/geometry/primitives/triangle.rs:11-44, :47-68 */
rmd_status rmd_probe_triangle_intersect(rmd_context *ctx, size_t n, const double *pos9, const double *ray6, int32_t *hit, double *t);
rmd_status rmd_probe_triangle_normal(rmd_context *ctx, size_t n, const double *pos9, const double *nrm9, const double *ray6,
                                     const double *t, double *n3);
/* src/trace.rs:408-416, :396-406, :286-296, :362-370, :380-382, :384-386 */
rmd_status rmd_probe_onb(rmd_context *ctx, size_t n, const double *n3, double *t3, double *b3);
rmd_status rmd_probe_cosine_hemisphere(rmd_context *ctx, size_t n, const double *r1, const double *r2, double *dir3, double *pdf);
rmd_status rmd_probe_importance_sample_ggx(rmd_context *ctx, size_t n, const double *reflect3, const double *rough, const double *r1,
                                           const double *r2, double *dir3);
rmd_status rmd_probe_ggx_distribution(rmd_context *ctx, size_t n, const double *n3, const double *h3, const double *rough, double *out);
rmd_status rmd_probe_geometry_smith(rmd_context *ctx, size_t n, const double *n3, const double *v3, const double *l3,
                                    const double *rough, double *out);
rmd_status rmd_probe_fresnel_schlick(rmd_context *ctx, size_t n, const double *cos_theta, const double *f0_3, double *out3);
/* The device's elementary functions as the kernels use them: IEEE sqrt (bit-exact) and the reduced-range sin / cos that
 * stand in for the reference's libm calls (src/trace.rs:291-293, :401-403; <= 2 ulp for |x| < 2^45). */
rmd_status rmd_probe_elementary(rmd_context *ctx, size_t n, const double *x, double *sqrt_out, double *sin_out, double *cos_out,
                                double *root_out, double *inv_root_out); /* root/inv_root: normalize()'s sqrt and 1.0 / sqrt, both bit-exact */
/* src/trace.rs:322-333 with the two jitter uniforms given explicitly (u2[2i], u2[2i+1]) */
rmd_status rmd_probe_primary_ray(rmd_context *ctx, size_t n, const rmd_camera *cam, const uint32_t *xy2, const double *u2, double *ray6);
/* core/src/scene.rs:54-74: obj[i] = object index or -1, sub[i] = triangle index for grid objects */
rmd_status rmd_probe_scene_intersect(rmd_context *ctx, const rmd_scene *scene, size_t n, const double *ray6, int32_t *obj, double *t,
                                     uint32_t *sub);
/* core/src/geometry/acc_grid.rs:89-185 on grid `g` of the scene */
rmd_status rmd_probe_grid_intersect(rmd_context *ctx, const rmd_scene *scene, uint32_t g, size_t n, const double *ray6, int32_t *hit,
                                    double *t, uint32_t *tri);
/* The same through the DEEP form of the walk — the form of the split / queued launches: the sphere pre-test in place, the ring of pairs in the wave's
 * carry area, walks put aside by cut_lanes / cut_round and taken up again from the carried DDA state (grid_walk.hpp).  One wave serves
 * `rays_per_wave` consecutive rays (a multiple of 64) the way the render loops do: a lane whose walk was put aside presents the same ray again, a lane
 * that is done takes the wave's next unserved ray, and the cuts reach only calls with at least 16 walkers (0 otherwise: every walk finishes).
 * cut_lanes = cut_round = 0: every call finishes every walk.  The wave's call loop is bounded; RMD_ERR_DEVICE_FAULT if a wave reaches the bound. */
rmd_status rmd_probe_grid_intersect_deep(rmd_context *ctx, const rmd_scene *scene, uint32_t g, size_t n, const double *ray6, uint32_t cut_lanes,
                                         uint32_t cut_round, uint32_t rays_per_wave, int32_t *hit, double *t, uint32_t *tri);
/* One sample per entry (src/trace.rs:199-200) through the render kernel's own code path:
 * rgb_out[3i..] = radiance of (xy2[2i], xy2[2i+1], sample[i]).  path_obj/path_sub (optional, n*17 each):
 * object index (-1 = miss) and triangle index per trace() depth, -2 beyond the path's end. */
rmd_status rmd_probe_trace_samples(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *cam, const rmd_settings *settings,
                                   size_t n, const uint32_t *xy2, const uint32_t *sample, double *rgb_out, int32_t *path_obj,
                                   uint32_t *path_sub);

/* Host only (no device needed): the sphere rmd_scene_create puts around a triangle for the grid walk's pre-test — out5 = centre (3), inflated
 * squared radius r2a, the triangle's distance-proportional allowance kb (a grid uses the largest of its triangles').  A (ray, triangle) pair whose
 * line passes the centre at more than sqrt(r2a + kb * |centre - origin|^2) is not run through triangle.rs:11-44; tests/test_pretest_allowance.py
 * checks, with the reference's test evaluated in binary64 on adversarial pairs, that no such pair would have passed it. */
rmd_status rmd_probe_triangle_sphere(size_t n, const double *pos9, double *out5);
/* The walk's pre-test on explicit (triangle, ray) pairs IN THE DEVICE'S OWN ARITHMETIC — the function the chunk loop calls (grid_walk.hpp:
 * sphere_pretest, fused multiply-adds included) — beside the device's triangle.rs:11-44 on the same pair.  sphere5 = centre (3), r2a, kb (the caller
 * chooses the allowance: the triangle's own, or a grid's largest); pass[i] = the pre-test lets the pair through, hit[i] / t[i] = the reference's test.
 * A pair with hit = 1 and pass = 0 would be a silently missed hit: tests/test_gpu_reference_pins.py asserts there is none among the adversarial
 * pairs of tests/test_pretest_allowance.py. */
/* Host only (no device needed): what the generation trips of the role-sorted spheres kernel visit for the primary rays of each 8x8 wave tile
 * (raymond_amd/csrc/primary_candidates.hpp — the function the kernel itself evaluates once per work item).  The scene is given as rmd_scene_create
 * would get it (objects, the number of grids, the value of RMD_TUNE_AXIS_PAIRS), the launch by its camera and settings; tiles4 = x0, y0, w, h per
 * tile (w, h in 1 .. 8).  launch3 = the launch's own visit mask (objects 0 .. 63), its axis pairs (three 10-bit fields: index + 1 of the later
 * plane of the pair of axis k, 0 = none) and whether the candidate sets are on for this launch; out2 = per tile the visit mask and the axis
 * pairs of its generation trips — the launch's own values when the sets are off.  tests/test_primary_candidates.py holds every object the
 * predicate drops to the oracle's primary rays. */
rmd_status rmd_probe_primary_candidates(const rmd_camera *cam, const rmd_settings *settings, const rmd_object *objects, uint32_t n_objects, uint32_t n_grids,
                                        int64_t axis_pairs_tunable, size_t n_tiles, const uint32_t *tiles4, uint64_t *launch3, uint64_t *out2);
/* Host only (no device needed): the tile class the role-sorted spheres kernel gives a work item of each 8x8 wave tile (raymond_amd/csrc/
 * primary_candidates.hpp: primary_one_wall, primary_wall_class — the functions the kernel itself evaluates once per work item).  Arguments as
 * rmd_probe_primary_candidates'.  launch1[0] = whether the classes are on for this launch (the candidate sets' conditions, RMD_TUNE_AXIS_PAIRS = 0
 * and black paths ended); out2 = per tile the class (0 general, 1 emitter, 2 black) and the object every primary ray of the tile hits (-1 for a
 * general tile).  tests/test_tile_classes.py holds both to the oracle. */
rmd_status rmd_probe_tile_classes(const rmd_camera *cam, const rmd_settings *settings, const rmd_object *objects, uint32_t n_objects, uint32_t n_grids,
                                  int64_t axis_pairs_tunable, size_t n_tiles, const uint32_t *tiles4, uint32_t *launch1, int32_t *out2);
/* Host only (no device needed): the form of a render launch as launch_render chooses it (raymond_amd/csrc/launch.hpp: LaunchPlan).  mode 0 = tiles
 * (direct), 1 = tiles buffered (split), 2 = list; grid = 1: the grid instantiation.  Per entry in5 = n_objects, mask_words_total, flags (1 = path
 * queues attached, 2 = persistence asked for — CUs and a work counter given —, 4 = chain_items, 8 = the squares asked for), n_waves, n_cus;
 * out8 = persistent, queued, chained, moments (the instantiation launched), waves per workgroup, workgroups, the per-wave LDS area charged, the
 * workgroup's dynamic LDS bytes.  tests/test_launch_plan.py checks it over every scene the library admits. */
rmd_status rmd_probe_launch_plan(uint32_t mode, uint32_t grid, size_t n, const uint32_t *in5, uint64_t *out8);
/* Host only: the sizes the plan is made of for instantiation (mode, grid): out8 = the LDS budget, sizeof(DevObject), the per-wave area of the
 * instantiation's unqueued kernels, the queued wave's area, waves of its persistent workgroup, waves of a one-wave-per-item workgroup of a scene with
 * grids, the spheres kernel's per-wave pool bytes (admission), the grids' mask budget bytes. */
rmd_status rmd_probe_launch_sizes(uint32_t mode, uint32_t grid, uint64_t *out8);
/* Host only (no device needed): the two-part work list of the role-sorted spheres kernel's split launches (raymond_amd/csrc/work_list.hpp; api.cpp:
 * plan_work_list).  Per entry in4 = wave slots, wave tiles, samples of the pass, the uniform rule's items per wave tile; out3 = n_whole (the wave tiles
 * that are one item each, first in the list), n_tail (the others) and k_tail (items per tail tile).  With ctx not null the plan is the one that
 * context — its wave slots, its tunables, a scene without grids — gives a pass of a render of that many wave tiles and samples: in4's first word is
 * then the samples of the pass asked about (0 = the render is one pass) and its last word is ignored.  tests/test_work_list.py walks the plans. */
rmd_status rmd_probe_work_plan(const rmd_context *ctx, size_t n, const uint32_t *in4, uint32_t *out3);
/* Host only: items first .. first + n - 1 of the list (n_tiles, n_whole, k_tail) of a pass of sample_count samples, by the mapping the kernel itself
 * evaluates (work_list.hpp: work_list_item): out5 = wave tile (n_tiles past the end of the list), first sample, sample count, parts of this tile,
 * 1 for a whole item; *n_items = the items of the list. */
rmd_status rmd_probe_work_items(uint32_t n_tiles, uint32_t n_whole, uint32_t k_tail, uint32_t sample_count, uint32_t first, size_t n, uint32_t *out5,
                                uint32_t *n_items);
/* Host only: the LDS layout of an uploaded scene — objects in the table, grids, and words of the grids' occupancy masks. */
rmd_status rmd_probe_scene_layout(const rmd_scene *scene, uint32_t *n_objects, uint32_t *n_grids, uint32_t *mask_words_total);
/* Host code only (no kernel runs): the launch rmd_intersect_rays would make for n_rays rays on an uploaded scene, from the functions its launcher
 * calls (raymond_amd/csrc/rays.hip: plan_rays_launch over rays_plan.hpp) — out6 = batches, waves per workgroup, workgroups, total waves, the
 * workgroup's dynamic LDS in bytes, the context's CU count.  n_rays above RMD_MAX_RAYS is refused. */
rmd_status rmd_probe_rays_plan(const rmd_scene *scene, uint64_t n_rays, uint64_t *out6);
/* Host code only (no kernel runs; the grids' records are copied back from the scene's device): what rmd_scene_create decided once for an uploaded
 * scene and every launch of it reads — out8 = n_grid_objects, regular, walk_steps_bound, axis_pairs, visit_mask, grid_mask, n_grids, 0 — and, for the
 * first n of its grids, shift_bits2 = mask_shift and mask_bits per grid.  tests/test_gpu_mesh_scenes.py asserts from it that a class of
 * tests/mesh_scenes.py reaches the state it names. */
rmd_status rmd_probe_scene_plan(const rmd_scene *scene, uint64_t *out8, size_t n, uint32_t *shift_bits2);
/* Host only: the device scratch block a denoise entry point carves (raymond_amd/csrc/denoise_host.hpp: denoise_scratch_layout — the function the entry
 * points themselves call).  form 0 = rmd_denoise[_guided], 1 = rmd_denoise_atrous, 2 = rmd_denoise_dual and its guided and region forms,
 * 3 = rmd_denoise_atrous_dual, 4 = rmd_denoise_atrous_dual_region, 5 = rmd_denoise_dual_select, 6 = rmd_tile_error_dual; guided = 1: the call has
 * features (form 5: a guided candidate); n_table: the entries of a region form's block tables (forms 2 and 4; ignored by the others).  Part p
 * (RMD_PROBE_SCRATCH_PARTS of them, in ScratchPart's order) has out3[3 * p] = 1 when the form holds it, then its offset and its length in bytes;
 * out3 therefore holds 3 * RMD_PROBE_SCRATCH_PARTS words — 45 since the slope planes became the fifteenth part (42 before: a caller sizes out3 by the constant);
 * *total = the block's bytes. */
#define RMD_PROBE_SCRATCH_FORMS 7u
#define RMD_PROBE_SCRATCH_PARTS 15u
rmd_status rmd_probe_denoise_scratch(uint32_t form, uint32_t width, uint32_t height, uint32_t n_rects, uint32_t guided, uint32_t n_cands, uint64_t n_table,
                                     uint64_t *out3, uint64_t *total);
/* ... of a _slope call (rmd_denoise_guided_slope, rmd_denoise_dual_guided_slope[_region], rmd_denoise_dual_select_slope): sloped = 1 when a slope the call
 * reads is > 0 — the forms 0, 2 and 5 with features then hold the seven slope planes, behind the feature planes; sloped = 0 is rmd_probe_denoise_scratch.
 * sloped = 2: an a-trous _slope call (rmd_denoise_atrous_slope, rmd_denoise_atrous_dual_slope[_region]) whose slope is > 0 — the forms 1, 3 and 4 with
 * features then hold the seven slope planes behind every other part, each of which keeps its offset.  (A value of its own: 1 leaves the a-trous forms alone.) */
rmd_status rmd_probe_denoise_scratch_slope(uint32_t form, uint32_t width, uint32_t height, uint32_t n_rects, uint32_t guided, uint32_t sloped, uint32_t n_cands,
                                           uint64_t n_table, uint64_t *out3, uint64_t *total);
/* Host only: the workgroup tile of the non-local-means kernels at a window (raymond_amd/csrc/denoise.hip: denoise_tile_width and denoise_lds_bytes — the
 * functions every launcher of rmd_denoise, rmd_denoise_dual, their guided, region and slope forms and rmd_denoise_dual_select sizes its launch with).
 * out4[0] = the tile width the launch takes (32 or 24), out4[1] = its dynamic LDS in bytes, out4[2] = the 32-wide tile's LDS in bytes, out4[3] = the LDS
 * budget in bytes.  RMD_ERR_INVALID_ARGUMENT past the header's limits (radius > 12, patch_radius > 4). */
rmd_status rmd_probe_denoise_tile(uint32_t radius, uint32_t patch_radius, uint64_t *out4);
/* The slope floors of the _slope denoise calls as the device makes them (raymond_amd/csrc/denoise.hip: feature_slope_kernel, through the launcher the entry
 * points call): fplanes7 = the seven planar per-pixel feature means f (W*H doubles each, HOST memory; a NaN in plane 0 marks a pixel that is not
 * feature-valid), mplanes7 = the seven planes m_j = (slope * slope) * (h_j + v_j) of include/raymond_hip.h, zeros at a pixel that is not feature-valid. */
rmd_status rmd_probe_feature_slope(rmd_context *ctx, const double *fplanes7, uint32_t width, uint32_t height, double slope, double *mplanes7);
/* The seven slope planes that this context's last rmd_denoise_atrous_dual_slope_region call with features, levels > 0 and slope > 0 left in the scratch it keeps
 * on the context, copied to mplanes7 (7 * W*H doubles, HOST memory; width and height must be that call's).  Only level 0's needed set is defined: the region's
 * rects grown by 2 * (2^levels - 2) pixels, clipped to the frame.  RMD_ERR_INVALID_ARGUMENT when no such call was made. */
rmd_status rmd_probe_atrous_region_slope_planes(rmd_context *ctx, uint32_t width, uint32_t height, double *mplanes7);
rmd_status rmd_probe_pretest_pairs(rmd_context *ctx, size_t n, const double *sphere5, const double *pos9, const double *ray6, int32_t *pass,
                                   int32_t *hit, double *t);

#ifdef __cplusplus
}
#endif
#endif
