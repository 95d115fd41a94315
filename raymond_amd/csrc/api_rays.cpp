// C-ABI implementation (include/raymond_hip.h) of the queries for caller-supplied rays: rmd_intersect_rays and its forms, rmd_camera_rays and the two
// buffer allocators.  Host code only; the kernels are in rays.hip, the launch's arithmetic in rays_plan.hpp.
#define RMD_WITH_HIP 1
#include "internal.hpp"
#include "launch.hpp"
#include "rays_plan.hpp"

using rmd::bind;

namespace {

// A camera and settings that make_params can be given where a call has none of its own: the scene's fields of RenderParams do not depend on them
const rmd_camera kNoCamera = {1u, 1u, 90.0, {0.0, 0.0, 0.0}, 1.0, 0.0};

rmd_settings no_settings() {
	rmd_settings st;
	std::memset(&st, 0, sizeof(st));
	st.bounce_limit = 1u, st.sample_count = 1u;
	return st;
}

// Refusals 1 and 2 of the header, which need no context: `name` is the call's own
rmd_status check_ray_buffers(rmd_context *ctx, const char *name, const void *scene_or_camera, const void *a, const void *b, uint64_t n_rays) {
	if (!scene_or_camera || (n_rays && (!a || !b))) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, std::string(name) + ": null pointer");
	if (n_rays > RMD_MAX_RAYS) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, std::string(name) + ": more than RMD_MAX_RAYS rays");
	return RMD_OK;
}

// The scene's refusals as a render makes them (api.cpp: check_render_args): the same two rules, the LDS one by the same expression
rmd_status check_scene_fits(rmd_context *ctx, const char *name, const rmd_scene *scene) {
	if (scene->ctx != ctx) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, std::string(name) + ": scene belongs to another context");
	if (rmd::render_lds_bytes(scene->n_objects, scene->mask_words_total, 1) + (scene->n_grids == 0u ? rmd::kSortPoolBytes : 0u) > rmd::kLdsBudgetBytes)
		return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, std::string(name) + ": object table + grid masks exceed the 160 KiB LDS of a CU");
	return RMD_OK;
}

rmd_status alloc_zeroed_doubles(rmd_context *ctx, const char *bad, uint64_t n_rays, size_t doubles_each, double **out_dev) {
	if (!out_dev || n_rays == 0u || n_rays > RMD_MAX_RAYS) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, bad);
	if (rmd_status s = bind(ctx)) return s;
	const size_t bytes = (size_t)n_rays * doubles_each * sizeof(double);
	RMD_HIP(ctx, hipMalloc((void **)out_dev, bytes));
	RMD_HIP(ctx, hipMemsetAsync(*out_dev, 0, bytes, ctx->stream));
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return RMD_OK;
}

} // namespace

extern "C" {

rmd_status rmd_ray_buffer_alloc(rmd_context *ctx, uint64_t n_rays, double **out_dev) {
	return alloc_zeroed_doubles(ctx, "rmd_ray_buffer_alloc: bad argument", n_rays, RMD_RAY_DOUBLES, out_dev);
}
rmd_status rmd_hit_buffer_alloc(rmd_context *ctx, uint64_t n_rays, rmd_ray_hit **out_dev) {
	return alloc_zeroed_doubles(ctx, "rmd_hit_buffer_alloc: bad argument", n_rays, RMD_HIT_DOUBLES, reinterpret_cast<double **>(out_dev));
}

rmd_status rmd_intersect_rays_async(rmd_context *ctx, const rmd_scene *scene, const double *rays_dev, uint64_t n_rays, rmd_ray_hit *hits_dev) {
	return rmd::guarded(ctx, "rmd_intersect_rays", [&]() -> rmd_status {
		if (rmd_status s = check_ray_buffers(ctx, "rmd_intersect_rays", scene, rays_dev, hits_dev, n_rays)) return s;
		if (rmd_status s = bind(ctx)) return s;
		if (rmd_status s = check_scene_fits(ctx, "rmd_intersect_rays", scene)) return s;
		if (n_rays == 0u) return RMD_OK;
		const rmd_settings st = no_settings();
		const rmd::RenderParams P = rmd::make_params(ctx, scene, &kNoCamera, &st);
		// (neither the context's events nor its launch record are touched: rmd_last_kernel_ms / rmd_last_launch_info keep describing the last render)
		RMD_HIP(ctx, rmd::launch_rays(ctx->stream, P, scene->d_objects, scene->d_grids, ctx->n_cus, rays_dev, n_rays, hits_dev));
		return RMD_OK;
	});
}

rmd_status rmd_intersect_rays(rmd_context *ctx, const rmd_scene *scene, const double *rays_dev, uint64_t n_rays, rmd_ray_hit *hits_dev) {
	if (rmd_status s = rmd_intersect_rays_async(ctx, scene, rays_dev, n_rays, hits_dev)) return s;
	return rmd_context_synchronize(ctx);
}

rmd_status rmd_intersect_rays_host(rmd_context *ctx, const rmd_scene *scene, const double *rays_host, uint64_t n_rays, rmd_ray_hit *hits_host) {
	return rmd::guarded(ctx, "rmd_intersect_rays_host", [&]() -> rmd_status {
		if (rmd_status s = check_ray_buffers(ctx, "rmd_intersect_rays_host", scene, rays_host, hits_host, n_rays)) return s;
		if (rmd_status s = bind(ctx)) return s;
		if (rmd_status s = check_scene_fits(ctx, "rmd_intersect_rays_host", scene)) return s;
		if (n_rays == 0u) return RMD_OK;
		const size_t ray_bytes = (size_t)n_rays * RMD_RAY_DOUBLES * sizeof(double), hit_bytes = (size_t)n_rays * sizeof(rmd_ray_hit);
		rmd::DeviceBuffer rays, hits; // freed however the call leaves; every path below waits for the stream first
		RMD_HIP(ctx, rays.alloc(ray_bytes));
		RMD_HIP(ctx, hits.alloc(hit_bytes));
		rmd_status s = rmd_framebuffer_upload(ctx, rays_host, rays.as<double>(), (size_t)n_rays * RMD_RAY_DOUBLES);
		if (!s) s = rmd_intersect_rays(ctx, scene, rays.as<double>(), n_rays, hits.as<rmd_ray_hit>());
		if (!s) s = rmd_framebuffer_download(ctx, hits.as<double>(), reinterpret_cast<double *>(hits_host), (size_t)n_rays * RMD_HIT_DOUBLES);
		if (s) (void)hipStreamSynchronize(ctx->stream);
		return s;
	});
}

rmd_status rmd_camera_rays(rmd_context *ctx, const rmd_camera *camera, const uint32_t *xy_host, const double *uv_host, uint64_t n_rays, double *rays_dev) {
	return rmd::guarded(ctx, "rmd_camera_rays", [&]() -> rmd_status {
		if (rmd_status s = check_ray_buffers(ctx, "rmd_camera_rays", camera, xy_host, rays_dev, n_rays)) return s;
		const uint32_t W = camera->backbuffer_width, H = camera->backbuffer_height;
		if (W == 0u || H == 0u || W > 65535u || H > 65535u) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_camera_rays: backbuffer size must be 1..65535 per axis");
		for (uint64_t i = 0; i < n_rays; i++)
			if (xy_host[2 * i] >= W || xy_host[2 * i + 1] >= H) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_camera_rays: pixel outside the frame");
		if (rmd_status s = bind(ctx)) return s;
		if (n_rays == 0u) return RMD_OK;
		const rmd_settings st = no_settings();
		const rmd::RenderParams P = rmd::make_params(ctx, nullptr, camera, &st);
		// [xy: 8 bytes an entry][uv: 16 bytes an entry], uploaded on an idle stream (the host arrays may be pageable) and freed after the wait below
		const size_t xy_bytes = (size_t)n_rays * 2 * sizeof(uint32_t), uv_bytes = uv_host ? (size_t)n_rays * 2 * sizeof(double) : 0;
		rmd::DeviceBuffer in;
		RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
		RMD_HIP(ctx, in.alloc(((xy_bytes + 15u) & ~(size_t)15u) + uv_bytes));
		uint32_t *d_xy = in.as<uint32_t>();
		double *d_uv = uv_host ? reinterpret_cast<double *>(in.as<unsigned char>() + ((xy_bytes + 15u) & ~(size_t)15u)) : nullptr;
		hipError_t e = hipMemcpyAsync(d_xy, xy_host, xy_bytes, hipMemcpyHostToDevice, ctx->stream);
		if (e == hipSuccess && d_uv) e = hipMemcpyAsync(d_uv, uv_host, uv_bytes, hipMemcpyHostToDevice, ctx->stream);
		if (e == hipSuccess) e = rmd::launch_camera_rays(ctx->stream, P, d_xy, d_uv, n_rays, rays_dev);
		const hipError_t w = hipStreamSynchronize(ctx->stream); // whatever was enqueued has ended before `in` goes
		RMD_HIP(ctx, e);
		RMD_HIP(ctx, w);
		return rmd::check_fault(ctx);
	});
}

} // extern "C"
