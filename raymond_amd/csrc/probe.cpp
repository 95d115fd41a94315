// Diagnostic entry points (include/raymond_hip_probe.h): pack host inputs, run one device
// function per element on the GPU, unpack.  Used by the parity tests only.
#define RMD_WITH_HIP 1
#include <cstring>
#include <vector>

#include "../../include/raymond_hip_probe.h"
#include "internal.hpp"
#include "launch.hpp"
#include "rays_plan.hpp"

namespace {

struct Column {
	const double *src;
	int width;
};

// rows of `in_stride` doubles built from the given columns; out rows of `out_stride` doubles
rmd_status run_probe(rmd_context *ctx, int op, size_t n, const std::vector<Column> &cols, int out_stride, std::vector<double> &out,
                     const rmd::RenderParams *params = nullptr) {
	if (!ctx) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "probe: null context");
	RMD_HIP(ctx, hipSetDevice(ctx->device));
	int in_stride = 0;
	for (const Column &c : cols) {
		if (!c.src && n) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "probe: null input array");
		in_stride += c.width;
	}
	std::vector<double> in(n * in_stride);
	for (size_t i = 0; i < n; i++) {
		double *row = in.data() + i * in_stride;
		for (const Column &c : cols) {
			std::memcpy(row, c.src + i * c.width, sizeof(double) * c.width);
			row += c.width;
		}
	}
	out.assign(n * out_stride, 0.0);
	if (n == 0) return RMD_OK;
	rmd::DeviceBuffer din, dout;
	RMD_HIP(ctx, din.alloc(in.size() * sizeof(double)));
	RMD_HIP(ctx, dout.alloc(out.size() * sizeof(double)));
	RMD_HIP(ctx, hipMemcpyAsync(din.as<void>(), in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	RMD_HIP(ctx, hipMemsetAsync(dout.as<void>(), 0, out.size() * sizeof(double), ctx->stream));
	rmd::RenderParams P;
	std::memset(&P, 0, sizeof(P));
	if (params) P = *params;
	RMD_HIP(ctx, rmd::launch_probe(ctx->stream, op, (uint32_t)n, din.as<const double>(), in_stride, dout.as<double>(), out_stride, P));
	RMD_HIP(ctx, hipMemcpyAsync(out.data(), dout.as<void>(), out.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return RMD_OK;
}

std::vector<double> widen(const uint32_t *src, size_t n) {
	std::vector<double> v(n);
	for (size_t i = 0; i < n; i++) v[i] = (double)src[i];
	return v;
}

rmd_status hit_t_probe(rmd_context *ctx, int op, size_t n, const double *shape, int shape_w, const double *ray6, int32_t *hit, double *t) {
	std::vector<double> out;
	if (rmd_status s = run_probe(ctx, op, n, {{shape, shape_w}, {ray6, 6}}, 2, out)) return s;
	for (size_t i = 0; i < n; i++) hit[i] = out[2 * i] != 0.0, t[i] = out[2 * i + 1];
	return RMD_OK;
}

void unpack(const std::vector<double> &out, int stride, int offset, int width, double *dst, size_t n) {
	for (size_t i = 0; i < n; i++) std::memcpy(dst + i * width, out.data() + i * stride + offset, sizeof(double) * width);
}

} // namespace

extern "C" {

rmd_status rmd_probe_philox4x32_10(rmd_context *ctx, size_t n, const uint32_t *ctr4, const uint32_t *key2, uint32_t *out4) {
	if (!ctr4 || !key2 || !out4) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "probe: null array");
	std::vector<double> c = widen(ctr4, n * 4), k = widen(key2, n * 2), out;
	if (rmd_status s = run_probe(ctx, rmd::PROBE_PHILOX, n, {{c.data(), 4}, {k.data(), 2}}, 4, out)) return s;
	for (size_t i = 0; i < n * 4; i++) out4[i] = (uint32_t)out[i];
	return RMD_OK;
}

rmd_status rmd_probe_block_uniforms(rmd_context *ctx, uint64_t seed, size_t n, const uint32_t *pixel, const uint32_t *sample,
                                    const uint32_t *block, double *out5) {
	if (!pixel || !sample || !block || !out5) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "probe: null array");
	std::vector<double> k0(n, (double)(uint32_t)seed), k1(n, (double)(uint32_t)(seed >> 32));
	std::vector<double> p = widen(pixel, n), s = widen(sample, n), d = widen(block, n), out;
	if (rmd_status st = run_probe(ctx, rmd::PROBE_UNIFORM, n, {{k0.data(), 1}, {k1.data(), 1}, {p.data(), 1}, {s.data(), 1}, {d.data(), 1}}, 5, out))
		return st;
	std::memcpy(out5, out.data(), n * 5 * sizeof(double));
	return RMD_OK;
}

rmd_status rmd_probe_sphere_intersect(rmd_context *ctx, size_t n, const double *sphere4, const double *ray6, int32_t *hit, double *t) {
	return hit_t_probe(ctx, rmd::PROBE_SPHERE_INTERSECT, n, sphere4, 4, ray6, hit, t);
}
rmd_status rmd_probe_sphere_normal(rmd_context *ctx, size_t n, const double *sphere4, const double *ray6, const double *t, double *n3) {
	std::vector<double> out;
	if (rmd_status s = run_probe(ctx, rmd::PROBE_SPHERE_NORMAL, n, {{sphere4, 4}, {ray6, 6}, {t, 1}}, 3, out)) return s;
	unpack(out, 3, 0, 3, n3, n);
	return RMD_OK;
}
rmd_status rmd_probe_plane_intersect(rmd_context *ctx, size_t n, const double *plane6, const double *ray6, int32_t *hit, double *t) {
	return hit_t_probe(ctx, rmd::PROBE_PLANE_INTERSECT, n, plane6, 6, ray6, hit, t);
}
rmd_status rmd_probe_aabb_intersect(rmd_context *ctx, size_t n, const double *aabb6, const double *ray6, int32_t *hit, double *t) {
	return hit_t_probe(ctx, rmd::PROBE_AABB_INTERSECT, n, aabb6, 6, ray6, hit, t);
}
rmd_status rmd_probe_triangle_intersect(rmd_context *ctx, size_t n, const double *pos9, const double *ray6, int32_t *hit, double *t) {
	return hit_t_probe(ctx, rmd::PROBE_TRIANGLE_INTERSECT, n, pos9, 9, ray6, hit, t);
}
rmd_status rmd_probe_triangle_normal(rmd_context *ctx, size_t n, const double *pos9, const double *nrm9, const double *ray6,
                                     const double *t, double *n3) {
	std::vector<double> out;
	std::vector<double> aux(n * 4);
	for (size_t i = 0; i < n; i++) rmd::triangle_aux(pos9 + i * 9, aux.data() + i * 4); // as rmd_scene_create does
	if (rmd_status s = run_probe(ctx, rmd::PROBE_TRIANGLE_NORMAL, n, {{pos9, 9}, {nrm9, 9}, {ray6, 6}, {t, 1}, {aux.data(), 4}}, 3, out)) return s;
	unpack(out, 3, 0, 3, n3, n);
	return RMD_OK;
}
rmd_status rmd_probe_onb(rmd_context *ctx, size_t n, const double *n3, double *t3, double *b3) {
	std::vector<double> out;
	if (rmd_status s = run_probe(ctx, rmd::PROBE_ONB, n, {{n3, 3}}, 6, out)) return s;
	unpack(out, 6, 0, 3, t3, n);
	unpack(out, 6, 3, 3, b3, n);
	return RMD_OK;
}
rmd_status rmd_probe_cosine_hemisphere(rmd_context *ctx, size_t n, const double *r1, const double *r2, double *dir3, double *pdf) {
	std::vector<double> out;
	if (rmd_status s = run_probe(ctx, rmd::PROBE_COSINE_HEMISPHERE, n, {{r1, 1}, {r2, 1}}, 4, out)) return s;
	unpack(out, 4, 0, 3, dir3, n);
	unpack(out, 4, 3, 1, pdf, n);
	return RMD_OK;
}
rmd_status rmd_probe_importance_sample_ggx(rmd_context *ctx, size_t n, const double *reflect3, const double *rough, const double *r1,
                                           const double *r2, double *dir3) {
	std::vector<double> out;
	if (rmd_status s = run_probe(ctx, rmd::PROBE_SAMPLE_GGX, n, {{reflect3, 3}, {rough, 1}, {r1, 1}, {r2, 1}}, 3, out)) return s;
	unpack(out, 3, 0, 3, dir3, n);
	return RMD_OK;
}
rmd_status rmd_probe_ggx_distribution(rmd_context *ctx, size_t n, const double *n3, const double *h3, const double *rough, double *o) {
	std::vector<double> out;
	if (rmd_status s = run_probe(ctx, rmd::PROBE_GGX_DISTRIBUTION, n, {{n3, 3}, {h3, 3}, {rough, 1}}, 1, out)) return s;
	unpack(out, 1, 0, 1, o, n);
	return RMD_OK;
}
rmd_status rmd_probe_geometry_smith(rmd_context *ctx, size_t n, const double *n3, const double *v3, const double *l3,
                                    const double *rough, double *o) {
	std::vector<double> out;
	if (rmd_status s = run_probe(ctx, rmd::PROBE_GEOMETRY_SMITH, n, {{n3, 3}, {v3, 3}, {l3, 3}, {rough, 1}}, 1, out)) return s;
	unpack(out, 1, 0, 1, o, n);
	return RMD_OK;
}
rmd_status rmd_probe_fresnel_schlick(rmd_context *ctx, size_t n, const double *cos_theta, const double *f0_3, double *out3) {
	std::vector<double> out;
	if (rmd_status s = run_probe(ctx, rmd::PROBE_FRESNEL_SCHLICK, n, {{cos_theta, 1}, {f0_3, 3}}, 3, out)) return s;
	unpack(out, 3, 0, 3, out3, n);
	return RMD_OK;
}
rmd_status rmd_probe_elementary(rmd_context *ctx, size_t n, const double *x, double *sqrt_out, double *sin_out, double *cos_out,
                                double *root_out, double *inv_root_out) {
	std::vector<double> out;
	if (rmd_status s = run_probe(ctx, rmd::PROBE_ELEMENTARY, n, {{x, 1}}, 5, out)) return s;
	unpack(out, 5, 0, 1, sqrt_out, n);
	unpack(out, 5, 1, 1, sin_out, n);
	unpack(out, 5, 2, 1, cos_out, n);
	unpack(out, 5, 3, 1, root_out, n);
	unpack(out, 5, 4, 1, inv_root_out, n);
	return RMD_OK;
}
rmd_status rmd_probe_primary_ray(rmd_context *ctx, size_t n, const rmd_camera *cam, const uint32_t *xy2, const double *u2, double *ray6) {
	if (!cam || !xy2) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "probe: null argument");
	rmd_settings st;
	std::memset(&st, 0, sizeof(st));
	rmd::RenderParams P = rmd::make_params(ctx, nullptr, cam, &st);
	std::vector<double> xy = widen(xy2, n * 2), out;
	if (rmd_status s = run_probe(ctx, rmd::PROBE_PRIMARY_RAY, n, {{xy.data(), 2}, {u2, 2}}, 6, out, &P)) return s;
	unpack(out, 6, 0, 6, ray6, n);
	return RMD_OK;
}

static rmd_status scene_probe(rmd_context *ctx, const rmd_scene *scene, int mode, uint32_t g, size_t n, const double *ray6, int32_t *a,
                              double *t, uint32_t *b) {
	if (!ctx || !scene || scene->ctx != ctx || !ray6 || !a || !t || !b) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	if (mode == 1 && g >= scene->n_grids) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "probe: grid index out of range");
	RMD_HIP(ctx, hipSetDevice(ctx->device));
	if (n == 0) return RMD_OK;
	rmd::DeviceBuffer din, dout;
	RMD_HIP(ctx, din.alloc(n * 6 * sizeof(double)));
	RMD_HIP(ctx, dout.alloc(n * 3 * sizeof(double)));
	RMD_HIP(ctx, hipMemcpyAsync(din.as<void>(), ray6, n * 6 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	RMD_HIP(ctx, rmd::launch_probe_scene(ctx->stream, mode, g, (uint32_t)n, scene->d_objects, scene->n_objects, scene->d_grids,
	                                     scene->n_grids, scene->mask_words_total, scene->axis_pairs, din.as<const double>(), dout.as<double>()));
	std::vector<double> out(n * 3);
	RMD_HIP(ctx, hipMemcpyAsync(out.data(), dout.as<void>(), out.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	for (size_t i = 0; i < n; i++) a[i] = (int32_t)out[3 * i], t[i] = out[3 * i + 1], b[i] = (uint32_t)out[3 * i + 2];
	return RMD_OK;
}

rmd_status rmd_probe_scene_intersect(rmd_context *ctx, const rmd_scene *scene, size_t n, const double *ray6, int32_t *obj, double *t,
                                     uint32_t *sub) {
	return scene_probe(ctx, scene, 0, 0, n, ray6, obj, t, sub);
}
rmd_status rmd_probe_grid_intersect(rmd_context *ctx, const rmd_scene *scene, uint32_t g, size_t n, const double *ray6, int32_t *hit,
                                    double *t, uint32_t *tri) {
	return scene_probe(ctx, scene, 1, g, n, ray6, hit, t, tri);
}

rmd_status rmd_probe_grid_intersect_deep(rmd_context *ctx, const rmd_scene *scene, uint32_t g, size_t n, const double *ray6, uint32_t cut_lanes,
                                         uint32_t cut_round, uint32_t rays_per_wave, int32_t *hit, double *t, uint32_t *tri) {
	if (!ctx || !scene || scene->ctx != ctx || !ray6 || !hit || !t || !tri) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	if (g >= scene->n_grids) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "probe: grid index out of range");
	if (rays_per_wave == 0u || rays_per_wave % 64u != 0u || rays_per_wave > (1u << 20) || cut_lanes > 255u || cut_round > 255u || n > 0x7FFFFFFFull)
		return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "probe: rays_per_wave must be a multiple of 64 up to 2^20, the cuts at most 255, n below 2^31");
	RMD_HIP(ctx, hipSetDevice(ctx->device));
	if (n == 0) return RMD_OK;
	rmd::DeviceBuffer din, dout, dstuck;
	RMD_HIP(ctx, din.alloc(n * 6 * sizeof(double)));
	RMD_HIP(ctx, dout.alloc(n * 3 * sizeof(double)));
	RMD_HIP(ctx, dstuck.alloc(sizeof(uint32_t)));
	RMD_HIP(ctx, hipMemcpyAsync(din.as<void>(), ray6, n * 6 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	RMD_HIP(ctx, hipMemsetAsync(dout.as<void>(), 0, n * 3 * sizeof(double), ctx->stream));
	RMD_HIP(ctx, hipMemsetAsync(dstuck.as<void>(), 0, sizeof(uint32_t), ctx->stream));
	RMD_HIP(ctx, rmd::launch_probe_grid_deep(ctx->stream, g, (uint32_t)n, scene->d_grids, scene->n_grids, scene->mask_words_total, din.as<const double>(), cut_lanes,
	                                         cut_round, rays_per_wave, scene->walk_steps_bound, dout.as<double>(), dstuck.as<uint32_t>()));
	std::vector<double> out(n * 3);
	uint32_t stuck = 0;
	RMD_HIP(ctx, hipMemcpyAsync(out.data(), dout.as<void>(), out.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	RMD_HIP(ctx, hipMemcpyAsync(&stuck, dstuck.as<void>(), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (stuck) return rmd::fail(ctx, RMD_ERR_DEVICE_FAULT, "probe: a wave of the DEEP walk reached its bound of walk calls with rays unfinished (it cannot: an internal fault)");
	for (size_t i = 0; i < n; i++) hit[i] = (int32_t)out[3 * i], t[i] = out[3 * i + 1], tri[i] = (uint32_t)out[3 * i + 2];
	return RMD_OK;
}

rmd_status rmd_probe_triangle_sphere(size_t n, const double *pos9, double *out5) {
	if (n != 0 && (!pos9 || !out5)) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	for (size_t i = 0; i < n; i++) {
		double kb = 0.0;
		rmd::triangle_sphere(pos9 + i * 9, out5 + i * 5, kb);
		out5[i * 5 + 4] = kb;
	}
	return RMD_OK;
}

rmd_status rmd_probe_primary_candidates(const rmd_camera *cam, const rmd_settings *settings, const rmd_object *objects, uint32_t n_objects, uint32_t n_grids,
                                        int64_t axis_pairs_tunable, size_t n_tiles, const uint32_t *tiles4, uint64_t *launch3, uint64_t *out2) {
	if (!cam || !settings || (n_objects && !objects) || !launch3 || (n_tiles != 0 && (!tiles4 || !out2))) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	return rmd::guarded(nullptr, "rmd_probe_primary_candidates", [&]() -> rmd_status {
		rmd::SceneObjects sc;
		if (rmd_status s = rmd::derive_scene_objects(nullptr, objects, n_objects, n_grids, axis_pairs_tunable, sc)) return s;
		// (the launch's parameters as make_params makes them; the scene's half of the switch as rmd_scene_create sets it)
		const rmd::RenderParams P = rmd::make_params(nullptr, nullptr, cam, settings);
		const bool on = (rmd::primary_cull_bits(sc.regular, n_grids, axis_pairs_tunable) & 1u) != 0u && rmd::primary_cull_allowed(P);
		launch3[0] = sc.visit_mask, launch3[1] = sc.axis_pairs, launch3[2] = on ? 1u : 0u;
		rmd::CullCamera cc;
		for (int a = 0; a < 3; a++) cc.pos[a] = P.cam_pos[a];
		cc.width = P.width, cc.height = P.height, cc.aspect = P.aspect, cc.tan_half_fov = P.tan_half_fov;
		for (size_t i = 0; i < n_tiles; i++) {
			const uint32_t *t = tiles4 + i * 4;
			uint64_t visit = sc.visit_mask;
			uint32_t pairs = sc.axis_pairs;
			if (on) {
				if (t[2] == 0u || t[2] > 8u || t[3] == 0u || t[3] > 8u || t[0] > 65535u || t[1] > 65535u) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "probe: a wave tile is 1..8 pixels a side");
				const rmd::TileCone cone = rmd::primary_tile_cone(cc, t[0], t[1], t[2], t[3]);
				for (uint32_t j = 0; j < n_objects && j < 64u; j++)
					if (sc.objs[j].geometry_kind == 1u && rmd::primary_sphere_cleared(cone, cc, sc.objs[j].origin, sc.objs[j].radius)) visit &= ~(1ull << j);
				pairs = rmd::primary_pairs_kept(cone, cc, sc.walls, sc.axis_pairs);
			}
			out2[i * 2] = visit, out2[i * 2 + 1] = pairs;
		}
		return RMD_OK;
	});
}

rmd_status rmd_probe_tile_classes(const rmd_camera *cam, const rmd_settings *settings, const rmd_object *objects, uint32_t n_objects, uint32_t n_grids,
                                  int64_t axis_pairs_tunable, size_t n_tiles, const uint32_t *tiles4, uint32_t *launch1, int32_t *out2) {
	if (!cam || !settings || (n_objects && !objects) || !launch1 || (n_tiles != 0 && (!tiles4 || !out2))) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	return rmd::guarded(nullptr, "rmd_probe_tile_classes", [&]() -> rmd_status {
		rmd::SceneObjects sc;
		if (rmd_status s = rmd::derive_scene_objects(nullptr, objects, n_objects, n_grids, axis_pairs_tunable, sc)) return s;
		// (the launch's parameters as make_params makes them for a scene: end_black_paths asks for a regular scene without a grid whose planes the
		// camera does not lie on, unless the settings say otherwise)
		const rmd::RenderParams P = rmd::make_params(nullptr, nullptr, cam, settings);
		std::vector<double> planes;
		for (uint32_t i = 0; i < n_objects; i++)
			if (objects[i].geometry_kind == RMD_GEOM_PLANE) planes.insert(planes.end(), objects[i].origin, objects[i].origin + 3), planes.insert(planes.end(), objects[i].normal, objects[i].normal + 3);
		const bool end_black = rmd::end_black_paths_rule(settings->flags, true, n_grids, sc.regular, rmd::camera_on_a_plane(planes, cam)); // (make_params' own rule)
		const bool on = rmd::primary_cull_bits(sc.regular, n_grids, axis_pairs_tunable) == 3u && rmd::primary_cull_allowed(P) && end_black;
		launch1[0] = on ? 1u : 0u;
		rmd::CullCamera cc;
		for (int a = 0; a < 3; a++) cc.pos[a] = P.cam_pos[a];
		cc.width = P.width, cc.height = P.height, cc.aspect = P.aspect, cc.tan_half_fov = P.tan_half_fov;
		for (size_t i = 0; i < n_tiles; i++) {
			const uint32_t *t = tiles4 + i * 4;
			out2[i * 2] = (int32_t)rmd::kTileGeneral, out2[i * 2 + 1] = -1;
			if (!on) continue;
			if (t[2] == 0u || t[2] > 8u || t[3] == 0u || t[3] > 8u || t[0] > 65535u || t[1] > 65535u) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "probe: a wave tile is 1..8 pixels a side");
			const rmd::TileCone cone = rmd::primary_tile_cone(cc, t[0], t[1], t[2], t[3]);
			uint64_t visit = sc.visit_mask;
			for (uint32_t j = 0; j < n_objects && j < 64u; j++)
				if (sc.objs[j].geometry_kind == 1u && rmd::primary_sphere_cleared(cone, cc, sc.objs[j].origin, sc.objs[j].radius)) visit &= ~(1ull << j);
			int k_alone = 0;
			bool faces_minus = false;
			const bool alone = rmd::primary_pair_alone(cone, cc, sc.walls, sc.axis_pairs, k_alone, faces_minus);
			uint32_t wall = 0u;
			const uint32_t cls = rmd::primary_tile_class(alone, k_alone, faces_minus, sc.walls, visit, n_objects, sc.objs.data(), wall); // (item_candidates' own call)
			out2[i * 2] = (int32_t)cls, out2[i * 2 + 1] = cls == rmd::kTileGeneral ? -1 : (int32_t)wall;
		}
		return RMD_OK;
	});
}

rmd_status rmd_probe_launch_plan(uint32_t mode, uint32_t grid, size_t n, const uint32_t *in5, uint64_t *out8) {
	if (mode > 2u || grid > 1u || (n != 0 && (!in5 || !out8))) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	for (size_t i = 0; i < n; i++) {
		const uint32_t *a = in5 + i * 5;
		const rmd::LaunchPlan L = rmd::plan_render_launch((int)mode, grid != 0u, a[0], a[1], (a[2] & 1u) != 0u, (a[2] & 2u) != 0u, (a[2] & 4u) != 0u,
		                                                  (a[2] & 8u) != 0u, a[3], a[4]);
		uint64_t *o = out8 + i * 8;
		o[0] = L.persistent, o[1] = L.queued, o[2] = L.chained, o[3] = L.moments, o[4] = L.waves_per_wg, o[5] = L.workgroups, o[6] = L.wave_lds, o[7] = L.lds;
	}
	return RMD_OK;
}

rmd_status rmd_probe_work_plan(const rmd_context *ctx, size_t n, const uint32_t *in4, uint32_t *out3) {
	if (n != 0 && (!in4 || !out3)) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	for (size_t i = 0; i < n; i++) {
		const uint32_t *a = in4 + i * 4;
		const rmd::WorkPlan w = ctx ? rmd::context_work_plan(ctx, false, a[1], a[2], a[0] ? a[0] : a[2]) : rmd::plan_work_list(a[0], a[1], a[2], a[3]);
		out3[i * 3] = w.n_whole, out3[i * 3 + 1] = w.n_tail, out3[i * 3 + 2] = w.k_tail;
	}
	return RMD_OK;
}

rmd_status rmd_probe_work_items(uint32_t n_tiles, uint32_t n_whole, uint32_t k_tail, uint32_t sample_count, uint32_t first, size_t n, uint32_t *out5,
                                uint32_t *n_items) {
	if (n_whole > n_tiles || k_tail == 0u || !n_items || (n != 0 && !out5)) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	*n_items = rmd::work_list_items(n_tiles, n_whole, k_tail);
	for (size_t i = 0; i < n; i++) {
		const rmd::WorkItem w = rmd::work_list_item(first + (uint32_t)i, n_tiles, n_whole, k_tail, sample_count);
		uint32_t *o = out5 + i * 5;
		o[0] = w.tile, o[1] = w.first, o[2] = w.count, o[3] = w.parts, o[4] = w.whole;
	}
	return RMD_OK;
}

rmd_status rmd_probe_launch_sizes(uint32_t mode, uint32_t grid, uint64_t *out8) {
	if (mode > 2u || grid > 1u || !out8) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	rmd::render_lds_sizes((int)mode, grid != 0u, out8);
	return RMD_OK;
}

static_assert(RMD_PROBE_SCRATCH_FORMS == rmd::kScratchForms && RMD_PROBE_SCRATCH_PARTS == rmd::kScratchParts, "include/raymond_hip_probe.h mirrors denoise_host.hpp");
rmd_status rmd_probe_denoise_scratch(uint32_t form, uint32_t width, uint32_t height, uint32_t n_rects, uint32_t guided, uint32_t n_cands, uint64_t n_table,
                                     uint64_t *out3, uint64_t *total) {
	if (form >= rmd::kScratchForms || guided > 1u || !out3 || !total) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	const rmd::ScratchLayout L = rmd::denoise_scratch_layout((rmd::ScratchForm)form, width, height, n_rects, guided != 0u, n_cands, (size_t)n_table);
	for (uint32_t p = 0; p < rmd::kScratchParts; p++) out3[3 * p] = L.used[p], out3[3 * p + 1] = L.offset[p], out3[3 * p + 2] = L.bytes[p];
	*total = L.total;
	return RMD_OK;
}
rmd_status rmd_probe_denoise_scratch_slope(uint32_t form, uint32_t width, uint32_t height, uint32_t n_rects, uint32_t guided, uint32_t sloped, uint32_t n_cands,
                                           uint64_t n_table, uint64_t *out3, uint64_t *total) {
	if (form >= rmd::kScratchForms || guided > 1u || sloped > 2u || !out3 || !total) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	const rmd::ScratchLayout L = rmd::denoise_scratch_layout((rmd::ScratchForm)form, width, height, n_rects, guided != 0u, n_cands, (size_t)n_table, sloped == 1u, sloped == 2u);
	for (uint32_t p = 0; p < rmd::kScratchParts; p++) out3[3 * p] = L.used[p], out3[3 * p + 1] = L.offset[p], out3[3 * p + 2] = L.bytes[p];
	*total = L.total;
	return RMD_OK;
}

rmd_status rmd_probe_denoise_tile(uint32_t radius, uint32_t patch_radius, uint64_t *out4) {
	if (radius > rmd::kDenoiseMaxRadius || patch_radius > rmd::kDenoiseMaxPatch || !out4) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	const uint32_t tw = rmd::denoise_tile_width(radius, patch_radius);
	out4[0] = tw, out4[1] = rmd::denoise_lds_bytes(tw, radius, patch_radius), out4[2] = rmd::denoise_lds_bytes(32u, radius, patch_radius), out4[3] = rmd::kLdsBudgetBytes;
	return RMD_OK;
}

rmd_status rmd_probe_feature_slope(rmd_context *ctx, const double *fplanes7, uint32_t width, uint32_t height, double slope, double *mplanes7) {
	if (!ctx || !fplanes7 || !mplanes7 || width == 0 || height == 0) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	RMD_HIP(ctx, hipSetDevice(ctx->device));
	const size_t bytes = (size_t)width * height * RMD_FEATURE_CHANNELS * sizeof(double);
	rmd::DeviceBuffer df, dm;
	RMD_HIP(ctx, df.alloc(bytes));
	RMD_HIP(ctx, dm.alloc(bytes));
	RMD_HIP(ctx, hipMemcpyAsync(df.as<void>(), fplanes7, bytes, hipMemcpyHostToDevice, ctx->stream));
	RMD_HIP(ctx, rmd::launch_feature_slope(ctx->stream, df.as<double>(), width, height, slope, dm.as<double>()));
	RMD_HIP(ctx, hipMemcpyAsync(mplanes7, dm.as<void>(), bytes, hipMemcpyDeviceToHost, ctx->stream));
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return RMD_OK;
}

rmd_status rmd_probe_atrous_region_slope_planes(rmd_context *ctx, uint32_t width, uint32_t height, double *mplanes7) {
	if (!ctx || !mplanes7 || ctx->atrous_region_slope_pixels == 0u || (size_t)width * height != ctx->atrous_region_slope_pixels)
		return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	RMD_HIP(ctx, hipSetDevice(ctx->device));
	const size_t bytes = ctx->atrous_region_slope_pixels * RMD_FEATURE_CHANNELS * sizeof(double);
	RMD_HIP(ctx, hipMemcpyAsync(mplanes7, ctx->atrous_region_scratch.as<unsigned char>() + ctx->atrous_region_slope_offset, bytes, hipMemcpyDeviceToHost, ctx->stream));
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return RMD_OK;
}

rmd_status rmd_probe_scene_layout(const rmd_scene *scene, uint32_t *n_objects, uint32_t *n_grids, uint32_t *mask_words_total) {
	if (!scene || !n_objects || !n_grids || !mask_words_total) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	*n_objects = scene->n_objects, *n_grids = scene->n_grids, *mask_words_total = scene->mask_words_total;
	return RMD_OK;
}

rmd_status rmd_probe_rays_plan(const rmd_scene *scene, uint64_t n_rays, uint64_t *out6) {
	if (!scene || !scene->ctx || !out6 || n_rays > RMD_MAX_RAYS) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	rmd::RenderParams P;
	std::memset(&P, 0, sizeof(P));
	P.n_objects = scene->n_objects, P.n_grids = scene->n_grids, P.mask_words_total = scene->mask_words_total; // what the plan reads of a launch's parameters
	rmd::RaysPlan plan;
	size_t lds = 0;
	if (!rmd::plan_rays_launch(P, n_rays, scene->ctx->n_cus, plan, &lds, nullptr)) return rmd::fail(nullptr, RMD_ERR_UNSUPPORTED, "probe: the scene's tables do not fit a CU's LDS");
	out6[0] = plan.batches, out6[1] = plan.waves_per_wg, out6[2] = plan.workgroups, out6[3] = plan.total_waves, out6[4] = lds, out6[5] = scene->ctx->n_cus;
	return RMD_OK;
}

rmd_status rmd_probe_scene_plan(const rmd_scene *scene, uint64_t *out8, size_t n, uint32_t *shift_bits2) {
	if (!scene || !scene->ctx || !out8 || (n && !shift_bits2) || n > scene->n_grids) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	rmd_context *ctx = scene->ctx;
	out8[0] = scene->n_grid_objects, out8[1] = scene->regular ? 1u : 0u, out8[2] = scene->walk_steps_bound, out8[3] = scene->axis_pairs;
	out8[4] = scene->visit_mask, out8[5] = scene->grid_mask, out8[6] = scene->n_grids, out8[7] = 0u;
	if (n == 0) return RMD_OK;
	std::vector<rmd::DevGrid> grids(n);
	RMD_HIP(ctx, hipSetDevice(ctx->device));
	RMD_HIP(ctx, hipMemcpyAsync(grids.data(), scene->d_grids, n * sizeof(rmd::DevGrid), hipMemcpyDeviceToHost, ctx->stream));
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	for (size_t g = 0; g < n; g++) shift_bits2[2 * g] = grids[g].mask_shift, shift_bits2[2 * g + 1] = grids[g].mask_bits;
	return RMD_OK;
}

rmd_status rmd_probe_pretest_pairs(rmd_context *ctx, size_t n, const double *sphere5, const double *pos9, const double *ray6, int32_t *pass, int32_t *hit,
                                   double *t) {
	if (n != 0 && (!sphere5 || !pos9 || !ray6 || !pass || !hit || !t)) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	std::vector<double> out;
	if (rmd_status s = run_probe(ctx, rmd::PROBE_PRETEST_PAIR, n, {{sphere5, 5}, {pos9, 9}, {ray6, 6}}, 3, out)) return s;
	for (size_t i = 0; i < n; i++) pass[i] = out[3 * i] != 0.0, hit[i] = out[3 * i + 1] != 0.0, t[i] = out[3 * i + 2];
	return RMD_OK;
}

rmd_status rmd_probe_trace_samples(rmd_context *ctx, const rmd_scene *scene, const rmd_camera *cam, const rmd_settings *settings,
                                   size_t n, const uint32_t *xy2, const uint32_t *sample, double *rgb_out, int32_t *path_obj,
                                   uint32_t *path_sub) {
	if (!ctx || !scene || scene->ctx != ctx || !cam || !settings || !xy2 || !sample || !rgb_out || (!path_obj != !path_sub))
		return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "probe: bad argument");
	if (settings->bounce_limit > RMD_MAX_BOUNCE_LIMIT) return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "probe: bounce_limit above RMD_MAX_BOUNCE_LIMIT");
	RMD_HIP(ctx, hipSetDevice(ctx->device));
	if (n == 0) return RMD_OK;
	std::vector<rmd::ListWork> list(n);
	for (size_t i = 0; i < n; i++) list[i] = rmd::ListWork{xy2[2 * i], xy2[2 * i + 1], sample[i], 0u};
	size_t n_pad = (n + 63) / 64 * 64;
	rmd::DeviceBuffer dl, drgb, dpo, dps;
	RMD_HIP(ctx, dl.alloc(n * sizeof(rmd::ListWork)));
	RMD_HIP(ctx, drgb.alloc(n_pad * 3 * sizeof(double)));
	RMD_HIP(ctx, hipMemcpyAsync(dl.as<void>(), list.data(), n * sizeof(rmd::ListWork), hipMemcpyHostToDevice, ctx->stream));
	if (path_obj) {
		RMD_HIP(ctx, dpo.alloc(n_pad * RMD_PATH_STRIDE * sizeof(int32_t)));
		RMD_HIP(ctx, dps.alloc(n_pad * RMD_PATH_STRIDE * sizeof(uint32_t)));
		std::vector<int32_t> init(n_pad * RMD_PATH_STRIDE, -2);
		RMD_HIP(ctx, hipMemcpyAsync(dpo.as<void>(), init.data(), init.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
		RMD_HIP(ctx, hipMemsetAsync(dps.as<void>(), 0, n_pad * RMD_PATH_STRIDE * sizeof(uint32_t), ctx->stream));
		RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	}
	rmd::RenderParams P = rmd::make_params(ctx, scene, cam, settings);
	P.n_work = (uint32_t)n;
	RMD_HIP(ctx, rmd::launch_render_list(ctx->stream, P, scene->d_objects, scene->d_grids, dl.as<const rmd::ListWork>(), drgb.as<double>(),
	                                     dpo.as<int32_t>(), dps.as<uint32_t>()));
	RMD_HIP(ctx, hipMemcpyAsync(rgb_out, drgb.as<void>(), n * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (path_obj) {
		RMD_HIP(ctx, hipMemcpyAsync(path_obj, dpo.as<void>(), n * RMD_PATH_STRIDE * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
		RMD_HIP(ctx, hipMemcpyAsync(path_sub, dps.as<void>(), n * RMD_PATH_STRIDE * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	}
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return RMD_OK;
}

} // extern "C"
